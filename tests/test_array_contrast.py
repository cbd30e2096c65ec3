"""The contrast of two runs along a receiver array (radiative3d_amd/contrasts/r3d_array_contrast.h) without a GPU: the host
build of the header against the definition restated in long double, within the header's own bounds; the known answers; the
three exact properties; the decibels and the gains against their formulas; the plan of ./main's options; and ./main's
refusals, which come before any node is built."""
import itertools
import math
import subprocess

import numpy as np
import pytest

from array_image_cases import WEIGHTS
from contrast_cases import (ARRAYS, BATCH_PAIRS, EA, EB, FIRST, GEOMETRIES, LD, N_BINS, NAN_BITS, ONLY_X, REGIONS, RHO, SCALES, SMOOTH, U,
                            WINDOWS, bits, bounds, case_regions, case_windows, host_array_contrast, host_contrasts, host_decibel,
                            jackknife_bound, jackknife_ld, restated, rows_as_blocks, same_bits, two_runs, two_sample_bound)
from cli_support import main_exe
from radiative3d_amd import Model, _ffi, contrast_decibel, contrast_gains
from tests.configs import halfspace


def close(got, want, bound, what):
    """got (float64) within `bound` of want (long double), NaN where and only where want is."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want)
    nan = np.isnan(want.astype(np.float64))
    assert (np.isnan(got) == nan).all(), what
    assert (bits(got[nan]) == NAN_BITS).all(), what
    err = np.abs(got.astype(LD)[~nan] - want[~nan])
    lim = np.broadcast_to(np.asarray(bound, dtype=LD), want.shape)[~nan]
    assert (err <= lim).all(), (what, float((err - lim).max()))


@pytest.mark.parametrize("n_bins", N_BINS)
def test_host_build_is_within_the_headers_bounds_of_the_long_double_restatement(n_bins):
    rng = np.random.default_rng(14000 + n_bins)
    runs = {pair: two_runs(*pair, n_bins, rng) for pair in BATCH_PAIRS}
    gains = {A: rng.uniform(0.5, 2.0, A) for A in ARRAYS}
    for (Ba, Bb), A, W, R, smooth, k in itertools.product(BATCH_PAIRS, ARRAYS, WINDOWS, REGIONS, SMOOTH, range(3)):
        if R and not W:
            continue
        xa, xb = runs[Ba, Bb]
        what = (n_bins, Ba, Bb, A, W, R, smooth, k)
        args = (xa, xb, FIRST, FIRST + A - 1, WEIGHTS[k], case_windows(A, W, n_bins), case_regions(A, R), gains[A], SCALES[k], smooth)
        got, want = host_array_contrast(*args), restated(*args)
        B, loo = max(Ba, Bb), Ba >= 2 and Bb >= 2
        e = bounds(B, n_bins, smooth, A)
        close(got["contrast"], want["contrast"], e["c"], what + ("contrast",))
        assert (np.abs(got["contrast"]) <= 1.0).all() and (got["lit"] == want["lit"]).all() and got["bad"] == 0
        if A == 3:
            assert (got["contrast"][1] == -1.0).all() and (bits(got["contrast"][2]) == 0).all() and got["lit"].tolist() == [1, 1, 0]
        close(got["window"][..., :2], want["window"][..., :2], e["E"] * want["window"][..., :2], what + ("E",))
        close(got["window"][..., RHO], want["window"][..., RHO], e["rho"] * np.nan_to_num(want["window"][..., RHO]), what + ("rho",))
        close(got["region"][..., :2], want["region"][..., :2], e["N"] * want["region"][..., :2], what + ("N",))
        close(got["region"][..., RHO], want["region"][..., RHO], e["rho_R"] * np.nan_to_num(want["region"][..., RHO]), what + ("rho_R",))
        if not loo:
            assert all(got[n] is None for n in ("contrast_se", "window_se", "region_se", "region_loo"))
            continue
        cse = want["contrast_se"]
        close(got["contrast_se"], cse, two_sample_bound(Ba, Bb, e["c"], cse, cse, cse), what + ("contrast_se",))
        for name, rel, ratio, top, qtop in (("window", "E", "rho", "window_loo_max", "ratio_loo_max"),
                                           ("region", "N", "rho_R", "region_loo_max", "region_ratio_max")):
            se = want[name + "_se"]
            for side, Bs in ((EA, Ba), (EB, Bb)):
                close(got[name + "_se"][..., side], se[..., side], jackknife_bound(Bs, e[rel] * want[top], se[..., side]),
                      what + (name, "se", side))
            s = np.nan_to_num(se[..., RHO].astype(np.float64))
            close(got[name + "_se"][..., RHO], se[..., RHO], two_sample_bound(Ba, Bb, e[ratio] * want[qtop], s, s, s), what + (name, "se rho"))
        q = want["region_loo"]
        close(got["region_loo"], q, e["rho_R"] * np.nan_to_num(q), what + ("region_loo",))


def test_the_geometry_of_the_row_sums_does_not_show_in_the_bits():
    rng = np.random.default_rng(14100)
    xa, xb = two_runs(3, 4, 130, rng)
    args = (xa, xb, FIRST, FIRST + 2, WEIGHTS[2], case_windows(3, 3, 130), case_regions(3, 2), rng.uniform(0.5, 2.0, 3), (1.0, 1.25), 2)
    one = host_array_contrast(*args, G=1)
    for G in GEOMETRIES[1:]:
        same_bits(host_array_contrast(*args, G=G), one)


def known_rows(n_bins, rng):
    """rows [4, n_bins] of few digits (every sum of them is exact) and the four receivers of the known answers: the test side
    equals the base, is half of it, is zero, and both are zero."""
    base = rng.integers(1, 64, (4, n_bins)).astype(np.float64)
    base[3] = 0.0
    test = base.copy()
    test[1] *= 0.5
    test[2] = 0.0
    return base, test


@pytest.mark.parametrize("B", (1, 2, 4))
def test_known_answers(B):
    rng = np.random.default_rng(14200)
    n_bins = 70
    base, test = known_rows(n_bins, rng)
    xa, xb = rows_as_blocks(np.repeat(base[None] / 4, B, axis=0)), rows_as_blocks(np.repeat(test[None] / 4, B, axis=0))
    got = host_array_contrast(xa, xb, 0, 3, ONLY_X, np.tile(np.array([[0, n_bins], [7, 66]], dtype=np.uint32), (4, 1, 1)), [(0, 0), (1, 1)],
                              np.ones(4))
    check_known(got, B)


def check_known(got, B):
    c, w = got["contrast"], got["window"]
    assert (bits(c[0]) == 0).all() and (w[0, :, RHO] == 1.0).all()
    assert (c[1] == -1.0 / 3.0).all() and (w[1, :, RHO] == 0.5).all()
    assert (c[2] == -1.0).all() and (bits(w[2, :, RHO]) == 0).all() and (w[2, :, EA] > 0).all()
    assert (bits(c[3]) == 0).all() and (bits(w[3, :, RHO]) == NAN_BITS).all() and (bits(w[3, :, :2]) == 0).all()
    assert got["lit"].tolist() == [1, 1, 1, 0] and got["bad"] == 0
    assert (got["region"][0, :, RHO] == 1.0).all() and (got["region"][1, :, RHO] == 0.5).all()
    if B >= 2:                                                     # equal batches, B <= 4: every se is zero exactly
        assert (bits(got["contrast_se"]) == 0).all() and (bits(got["window_se"][:3]) == 0).all() and (bits(got["region_se"]) == 0).all()
        assert (bits(got["window_se"][3, :, RHO]) == NAN_BITS).all() and (bits(got["window_se"][3, :, :2]) == 0).all()
        assert (got["region_loo"][0] == 1.0).all() and (got["region_loo"][1] == 0.5).all()
    else:
        assert got["contrast_se"] is None and got["region_loo"] is None


def test_swapping_the_sides_negates_the_contrast_and_keeps_its_se():
    rng = np.random.default_rng(14300)
    for (Ba, Bb), smooth in itertools.product(((2, 3), (64, 2), (1, 1)), (0, 3)):
        xa, xb = two_runs(Ba, Bb, 130, rng)
        bins = case_windows(3, 2, 130)
        ab = host_array_contrast(xa, xb, FIRST, FIRST + 2, WEIGHTS[2], bins, scale=(1.0, 1.25), smooth=smooth)
        ba = host_array_contrast(xb, xa, FIRST, FIRST + 2, WEIGHTS[2], bins, scale=(1.25, 1.0), smooth=smooth)
        zero = ab["contrast"] == 0
        assert (bits(ba["contrast"][~zero]) == bits(-ab["contrast"][~zero])).all() and (~zero).sum() > 130
        assert (bits(ba["contrast"][zero]) == 0).all() and (bits(ab["contrast"][zero]) == 0).all()       # (a zero stays +0.0)
        assert (ab["lit"] == ba["lit"]).all()
        assert (bits(ab["window"][..., EA]) == bits(ba["window"][..., EB])).all() and (bits(ab["window"][..., EB]) == bits(ba["window"][..., EA])).all()
        if Ba >= 2 and Bb >= 2:
            assert (bits(ab["contrast_se"]) == bits(ba["contrast_se"])).all() and (ab["contrast_se"] > 0).any()
            assert (bits(ab["window_se"][..., EA]) == bits(ba["window_se"][..., EB])).all()


def test_a_power_of_two_on_both_scales_changes_no_bit():
    rng = np.random.default_rng(14400)
    xa, xb = two_runs(3, 4, 129, rng)
    args = (xa, xb, FIRST, FIRST + 2, WEIGHTS[2], case_windows(3, 3, 129), case_regions(3, 2), rng.uniform(0.5, 2.0, 3))
    one = host_array_contrast(*args, scale=(1.0, 1.25), smooth=3)
    for p in (2.0, 0.125, 2.0 ** 40):
        two = host_array_contrast(*args, scale=(p, 1.25 * p), smooth=3)
        for name in ("contrast", "contrast_se", "region_loo"):
            assert (bits(one[name]) == bits(two[name])).all(), name
        for name in ("window", "window_se", "region", "region_se"):
            assert (bits(one[name][..., RHO]) == bits(two[name][..., RHO])).all(), name
            assert (bits(one[name][..., :2] * p) == bits(two[name][..., :2])).all(), name
    assert np.isfinite(one["region_loo"]).any() and (one["contrast_se"] > 0).any()


@pytest.mark.parametrize("B", (2, 3, 4))
def test_equal_batches_give_zero_se(B):
    rng = np.random.default_rng(14500 + B)
    one_a, one_b = rng.lognormal(0.0, 2.0, (1, 4, 100, 5)), rng.lognormal(0.0, 2.0, (1, 4, 100, 5))
    xa, xb = np.repeat(one_a, B, axis=0), np.repeat(one_b, 6 - B, axis=0)
    got = host_array_contrast(xa, xb, 1, 3, WEIGHTS[2], case_windows(3, 2, 100), case_regions(3, 2), rng.uniform(0.5, 2.0, 3), (1.0, 0.75), 3)
    for name in ("contrast_se", "window_se", "region_se"):
        assert (bits(got[name]) == 0).all(), name
    assert (np.abs(got["contrast"]) > 0).all()


def test_decibels_and_gains_against_their_formulas():
    rng = np.random.default_rng(14600)
    Ba, Bb = 5, 3
    loo = rng.uniform(0.2, 0.4, Ba + Bb)
    rho = 0.3
    d = 10 * np.log10(loo.astype(LD))
    want_se = np.sqrt(jackknife_ld(d[:Ba]) ** 2 + jackknife_ld(d[Ba:]) ** 2)
    for db, se in (host_decibel(Ba, Bb, rho, loo), contrast_decibel(Ba, Bb, rho, loo)):
        assert abs(db - 10 * math.log10(rho)) <= 8 * U * abs(db) and abs(se - float(want_se)) <= 64 * U * 10 / rho + 16 * U * se
    assert host_decibel(Ba, Bb, rho, loo) == contrast_decibel(Ba, Bb, rho, loo)
    db, se = contrast_decibel(Ba, Bb, rho)
    assert db == host_decibel(Ba, Bb, rho, None)[0] and math.isnan(se)
    db, se = contrast_decibel(1, 1, rho, loo[:2])
    assert abs(db - 10 * math.log10(rho)) <= 8 * U * abs(db) and math.isnan(se)
    bad = loo.copy()
    bad[6] = 0.0
    for args in ((Ba, Bb, 0.0, loo), (Ba, Bb, math.nan, loo), (Ba, Bb, rho, bad), (Ba, Bb, -1.0, None)):
        assert all(math.isnan(v) for v in contrast_decibel(*args))
    with pytest.raises(ValueError):
        contrast_decibel(Ba, Bb, rho, loo[:3])
    r = np.array([50.0, 100.0, 150.0, 400.0])
    for q in (0.0, 0.5, 1.0, -2.0):
        g = contrast_gains(r, 100.0, q)
        assert np.allclose(g, (r / 100.0) ** q, rtol=4 * U, atol=0) and (q != 0.0 or (g == 1.0).all())
        h = np.zeros(4)
        assert host_contrasts().contrast_gains_host(4, r.ctypes.data, 100.0, q, h.ctypes.data) == 0 and (h == g).all()
    for args in ((r, 0.0, 1.0), (r, math.nan, 1.0), (r, 100.0, math.inf), (np.array([0.0, 1.0]), 1.0, -1.0)):
        with pytest.raises(ValueError, match="r3d_contrast_gains: "):
            contrast_gains(*args)


# ---- the plan of ./main's options, and its refusals ---------------------------------------------------------------------------------
TEST_ARGS = "0.8,0.01,1.0,0.5,100,0.8,0.01,1.0,0.5,100,6.40,3.63,2.83,-60,6.40,3.63,2.83,-400"   # both layers' Q: 1000 -> 100
CONTRAST = ["--array-contrast=2", "--contrast-model-args=" + TEST_ARGS, "--contrast-array=48,95", "--contrast-axes=1,1,0",
            "--contrast-windows=6.4,3.0,3.63,2.0", "--contrast-regions=0,100,150,260", "--contrast-range-power=0.5"]
RUN = ["--num-phonons=3K", "--seed=77", "--error-batches=4"]


def test_the_plan_has_the_window_rule_and_the_regions_of_the_distances():
    from radiative3d_amd import window_bins
    model = Model(halfspace(3) + RUN + CONTRAST)
    plan = model.contrast_plan()
    n_bins, dt = model.n_bins, model.desc.params.time_per_bin
    r = plan["distances"]
    assert (plan["first"], plan["last"], plan["smooth"], plan["axes"]) == (48, 95, 2, (1.0, 1.0, 0.0))
    assert plan["test_args"] == [float(v) for v in TEST_ARGS.split(",")] and plan["seed"] == 78 and plan["num_phonons"] == 3000
    assert plan["velocities"].tolist() == [[6.4, 3.0], [3.63, 2.0]] and plan["regions_km"].tolist() == [[0.0, 100.0], [150.0, 260.0]]
    assert r.shape == (48,) and abs(r[-1] - 260.0) < 1e-9 and (np.diff(r) > 0).all() and plan["range_power"] == 0.5
    for i in range(48):
        for w, (v1, v2) in enumerate(plan["velocities"]):
            b0, b1, cut = window_bins(dt, n_bins, r[i], v1, 0.0, 0.0, r[i] / v2 - r[i] / v1)
            assert (b0, b1, cut) == (plan["bins"][i, w, 0], plan["bins"][i, w, 1], bool(plan["clipped"][i, w])), (i, w)
    assert (plan["bins"][:, :, 1] <= n_bins).all() and (plan["bins"][-1, :, 1] > plan["bins"][-1, :, 0]).all()
    for (lo, hi), (i0, i1) in zip(plan["regions_km"], plan["regions"]):
        inside = np.flatnonzero((r >= lo) & (r <= hi))
        assert (i0, i1) == (inside[0], inside[-1]) and inside.size == i1 - i0 + 1
    assert plan["r_ref"] == 0.5 * (r[0] + r[-1]) and (plan["gain"] == contrast_gains(r, plan["r_ref"], 0.5)).all()
    assert Model(halfspace(3) + RUN).contrast_plan() is None
    flat = Model(halfspace(3) + RUN + CONTRAST[:2]).contrast_plan()
    assert (flat["first"], flat["last"], flat["smooth"]) == (0, model.n_seismometers - 1, 2) and (flat["gain"] == 1.0).all()
    assert flat["bins"].shape == (model.n_seismometers, 0, 2) and flat["regions"].shape == (0, 2)
    with pytest.raises(RuntimeError, match="no receiver of the array lies between"):
        Model(halfspace(3) + RUN + CONTRAST[:5] + ["--contrast-regions=300,400"]).contrast_plan()


@pytest.mark.parametrize("extra, message", (
    (["--contrast-model-args=" + TEST_ARGS], "--contrast-model-args needs --array-contrast"),
    (["--array-contrast"], "--array-contrast needs --contrast-model-args=a,b,..."),
    (["--contrast-array=0,3"], "--contrast-array needs --array-contrast"),
    (CONTRAST[:2] + ["--gpus=2"], "--array-contrast runs on one device: --gpus / --devices name 2 shards"),
    (CONTRAST[:2] + ["--devices=0,0"], "--array-contrast runs on one device"),
    (CONTRAST[:2] + ["--slant-stack=0,0.3,4"], "--array-contrast cannot be combined with --slant-stack"),
    (CONTRAST[:2] + ["--lapse-windows"], "--array-contrast cannot be combined with --lapse-windows"),
    (CONTRAST[:2] + ["--ttimage"], "--array-contrast cannot be combined with --ttimage"),
    (CONTRAST[:2] + ["--envelope-shape"], "--array-contrast cannot be combined with --envelope-shape"),
    (CONTRAST[:2] + ["--target-error=0.1,0.9,16,4"], "--array-contrast cannot be combined with --target-error"),
    (CONTRAST[:2] + ["--reports=ALL_ON"], "--array-contrast cannot be combined with --reports"),
    (CONTRAST[:2] + ["--contrast-regions=0,100"], "--contrast-regions needs --contrast-windows"),
    (CONTRAST[:2] + ["--contrast-windows=3.0,6.4"], "every pair must be finite with V1 > V2 > 0"),
    (CONTRAST[:2] + ["--contrast-num-phonons=3"], "the test run's 3 histories are fewer than the 4 batches"),
    (["--array-contrast=65", "--contrast-model-args=" + TEST_ARGS], "SMOOTH, the three-point smoothing passes, must be 0 .. 64"),
    (CONTRAST[:2] + ["--contrast-array=48,144"], "--contrast-array=48,144: the model has the seismometers 0 .. 143."),
    (CONTRAST[:5] + ["--contrast-regions=300,400"], "--contrast-regions: no receiver of the array lies between")))
def test_main_refuses_each_bad_combination_before_a_node_is_built(tmp_path, extra, message):
    """What the options rule out is told when they are read, what needs the model when the job is made (make_batch_job) --
    BEFORE a node is built and a history runs: no GPU is needed to be told."""
    r = subprocess.run([main_exe()] + halfspace(3) + ["--host-tables", "--num-phonons=1K", "--error-batches=4", f"--output-dir={tmp_path}"] + extra,
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stdout[-2000:]
    assert message in r.stdout and ("** Error" in r.stdout), r.stdout[-2000:]
    assert "__BEGINNING_SIMULATION__" not in r.stdout
    assert "no HIP device" not in r.stdout
    assert not list(tmp_path.iterdir())


def test_main_refuses_the_contrast_without_error_batches(tmp_path):
    r = subprocess.run([main_exe()] + halfspace(3) + ["--host-tables", "--num-phonons=1K", f"--output-dir={tmp_path}"] + CONTRAST[:2],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--array-contrast needs --error-batches=B" in r.stdout, r.stdout[-2000:]
    assert "no HIP device" not in r.stdout and not list(tmp_path.iterdir())
