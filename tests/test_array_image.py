"""The arithmetic of the travel-time image (radiative3d_amd/arrays/r3d_array_image.h) as the host compiler builds it: the
launch geometry does not show in the bits; pixels and their jackknife errors against the reference's scripts restated in
long double, within the header's derived bounds; the batches' row sums against the window header; the edge cases; the
power-law fit.  No GPU."""
import math

import numpy as np
import pytest

from array_image_cases import (BATCHES, CURVE, FIRST, GEOMETRIES, LD_U, LEGACY, N_BINS, S_ALL, U, WEIGHTS, array_blocks,
                               curve_values, exact_row_sum, host_array_image, host_powerlaw, pixel_eps, restated_image,
                               restated_powerlaw_jackknife)
from window_cases import host_window_sums


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    for key in ("image", "image_se", "row_sum", "peak"):
        if a[key] is None:
            assert b[key] is None
        else:
            assert (bits(a[key]) == bits(b[key])).all(), key
    assert (a["peak_bin"] == b["peak_bin"]).all() and (a["lit"] == b["lit"]).all() and a["bad"] == b["bad"]


@pytest.mark.parametrize("n_bins", N_BINS)
def test_the_geometry_changes_no_bit(n_bins):
    rng = np.random.default_rng(6000 + n_bins)
    for B in (1, 3, 64):
        x = array_blocks(B, n_bins, rng)
        curve = curve_values(3, rng)
        for mode in (LEGACY, CURVE):
            want = host_array_image(x, FIRST, FIRST + 2, WEIGHTS[2], 1, mode, 0.3, curve, n_bins * 0.5, G=1)
            for G in GEOMETRIES[1:]:
                same(want, host_array_image(x, FIRST, FIRST + 2, WEIGHTS[2], 1, mode, 0.3, curve, n_bins * 0.5, G=G))


def check_against_restatement(x, first, last, weights, k, mode, rho, curve, Tw):
    B, _, n_bins = x.shape[:3]
    got = host_array_image(x, first, last, weights, k, mode, rho, curve, Tw)
    image, se, peak, loo_max = restated_image(x, first, last, weights, k, mode, rho, curve, Tw)
    eps, d = pixel_eps(B, n_bins, k, mode)
    ref = d * 2 * LD_U                                   # the restatement's own roundings, in its own unit
    err = np.abs(got["image"].astype(np.longdouble) - image)
    assert (err <= (eps + ref) * image).all(), (B, n_bins, k, mode, rho, float((err / np.maximum(image, 1e-300)).max()), eps)
    worst = float((err[image > 0] / image[image > 0]).max() / eps) if (image > 0).any() else 0.0
    assert (np.abs(got["peak"].astype(np.longdouble) - peak) <= (B + 7) * 2 * U * peak).all()
    worst_se = 0.0
    if B >= 2:
        lim = 2 * B ** 1.5 * (eps + ref) * loo_max + (B + 4) * (eps + ref) * se
        err = np.abs(got["image_se"].astype(np.longdouble) - se)
        assert (err <= lim).all(), (B, n_bins, k, mode, rho, float((err - lim).max()))
        worst_se = float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0
    return worst, worst_se


@pytest.mark.parametrize("k", [0, 1, 2])
def test_pixels_and_errors_against_the_scripts_restated_in_long_double(k):
    """Gammas 1, 2, 4; rho 0, 0.3, 1 and CURVE mode; every B and n_bins of the kernel's shapes.  The bounds are the header's:
    eps = d u / (1 - 2 d u) relative for a pixel, 2 B^1.5 eps max_j img_(j) + (B + 4) eps se for its error, each widened by
    the long-double restatement's own d roundings of 2^-64."""
    rng = np.random.default_rng(6100 + k)
    worst = worst_se = 0.0
    for n_bins in N_BINS:
        for B in BATCHES:
            x = array_blocks(B, n_bins, rng)
            curve = curve_values(3, rng)
            weights = WEIGHTS[(n_bins + B) % 3]
            for mode, rho in ((LEGACY, 0.0), (LEGACY, 0.3), (LEGACY, 1.0), (CURVE, 0.0)):
                a, b = check_against_restatement(x, FIRST, FIRST + 2, weights, k, mode, rho, curve, n_bins * 0.5)
                worst, worst_se = max(worst, a), max(worst_se, b)
    print(f"gamma 2^{k}: worst pixel error / bound = {worst:.3f}, worst se error / bound = {worst_se:.4f}")


@pytest.mark.parametrize("n_bins", N_BINS)
def test_batch_row_sums_are_the_window_sums_of_the_full_trace(n_bins):
    rng = np.random.default_rng(6200 + n_bins)
    for B in (1, 3):
        x = array_blocks(B, n_bins, rng)
        for weights in WEIGHTS:
            got = host_array_image(x, FIRST, FIRST + 2, weights, 1)["row_sum"]
            bins = np.broadcast_to(np.array([0, n_bins], dtype=np.uint32), (S_ALL, 1, 2)).copy()
            want, _, bad = host_window_sums(x, bins, weights)
            assert bad == 0 and (bits(got) == bits(want[:, FIRST:FIRST + 3, 0])).all()
            # ... and lie within the window header's bound of the exact rational sum
            d = -(-n_bins // 64) + 10
            for j in range(B):
                exact = exact_row_sum(x[j, FIRST], weights)
                assert abs(float(got[j, 0]) - exact) <= d * U / (1 - d * U) * exact


def test_equal_batches_give_se_zero_exactly():
    """For B <= 4 the leave-one-out rows of equal batches coincide whatever the values (L_j + R_j is the same additions up to
    commuting); for larger B where the batches' sums are exact: values of few digits."""
    rng = np.random.default_rng(6300)
    for B in (2, 3, 4, 64):
        one = rng.lognormal(0.0, 3.0, (1, S_ALL, 70, 5))
        if B > 4:
            one = np.ldexp(rng.integers(1, 1 << 20, one.shape).astype(np.float64), -10)
        x = np.repeat(one, B, axis=0)
        for mode in (LEGACY, CURVE):
            for k in (0, 1, 2):
                got = host_array_image(x, FIRST, FIRST + 2, WEIGHTS[0], k, mode, 0.3, curve_values(3, rng), 35.0)
                assert (bits(got["image_se"]) == 0).all(), (B, mode, k)
                assert (got["image"] > 0).all() and (got["lit"] == 1).all()


def test_a_zero_row_is_dead_with_positive_zero_pixels():
    rng = np.random.default_rng(6400)
    x = array_blocks(3, 65, rng)
    for k in (0, 1, 2):
        got = host_array_image(x, FIRST, FIRST + 2, WEIGHTS[0], k)
        assert got["lit"].tolist() == [1, 1, 0]
        assert (bits(got["image"][2]) == 0).all() and (bits(got["image_se"][2]) == 0).all()
        assert bits(got["peak"][2]) == 0 and got["peak_bin"][2] == 0 and (bits(got["row_sum"][:, 2]) == 0).all()
    # weights that silence a row's only components do the same
    got = host_array_image(x, FIRST, FIRST + 1, (0, 0, 0, 0, 0), 1)
    assert (got["lit"] == 0).all() and (bits(got["image"]) == 0).all()


def test_a_tied_peak_takes_the_first_bin():
    rng = np.random.default_rng(6500)
    for n_bins in (63, 64, 65, 130):
        for B in (1, 3, 64):
            x = array_blocks(B, n_bins, rng)
            for G in (1, 4, 64):
                got = host_array_image(x, FIRST, FIRST, WEIGHTS[2], 1, G=G)
                assert got["peak_bin"][0] == n_bins // 3 and (2 * n_bins) // 3 > n_bins // 3
                # (both bins hold the peak, to the bit, and the pixels there are the row's largest)
                row = got["image"][0]
                assert bits(row[n_bins // 3]) == bits(row[(2 * n_bins) // 3]) and row[n_bins // 3] == row.max()


def test_a_row_lit_by_one_batch_has_a_dead_leave_one_out_row_and_a_finite_error():
    rng = np.random.default_rng(6600)
    B, n_bins = 5, 70
    x = array_blocks(B, n_bins, rng)
    x[:, FIRST] = 0.0
    x[2, FIRST] = rng.lognormal(0.0, 3.0, (n_bins, 5))
    for mode in (LEGACY, CURVE):
        got = host_array_image(x, FIRST, FIRST, WEIGHTS[0], 1, mode, 0.3, [3.0], 35.0)
        img, se = got["image"][0], got["image_se"][0]
        assert got["lit"][0] == 1 and (img > 0).all() and np.isfinite(se).all() and (se > 0).all()
        # four leave-one-out rows are the row itself scaled by B / (B - 1), one is dead (+0.0): in LEGACY mode, where a
        # row's scale cancels, the jackknife is that of (p, p, 0, p, p): mean 0.8 p, se = 0.8 p
        if mode == LEGACY:
            assert np.allclose(se, img * math.sqrt((B - 1) / B * (4 * 0.2 ** 2 + 0.8 ** 2)), rtol=1e-12, atol=0)
        image, ref_se, _, _ = restated_image(x, FIRST, FIRST, WEIGHTS[0], 1, mode, 0.3, [3.0], 35.0)
        assert np.allclose(se, ref_se[0].astype(np.float64), rtol=1e-12, atol=0)


# ---- the fit ------------------------------------------------------------------------------------------------------------
FIT_SEEDS = range(40)
FIT_TOLERANCE = 1e-10


def fit_case(seed):
    rng = np.random.default_rng(6700 + seed)
    A = int(rng.integers(8, 49))
    r0 = float(rng.uniform(5.0, 40.0))
    r1 = r0 * float(rng.uniform(10.0, 30.0))              # ranges over more than a decade
    B = int(rng.integers(2, 13))
    X = r0 + np.arange(A) * ((r1 - r0) / (A - 1))
    q = float(rng.uniform(-3.0, -0.5))
    y = 10.0 ** rng.uniform(-3, 3) * X ** q * rng.lognormal(0.0, 0.3, (B, A)) / B
    ibegin = int(rng.integers(1, A - 6))
    iend = int(rng.integers(ibegin + 7, A + 1))           # at least 8 points
    return A, r0, r1, y, ibegin, iend


def fit_deviation(seed):
    A, r0, r1, y, ibegin, iend = fit_case(seed)
    rc, lnc, q, se_c, se_q, total = host_powerlaw(y, r0, r1, ibegin, iend)
    assert rc == 0 and iend - ibegin + 1 >= 8 and r1 / r0 >= 10
    want = [float(v) for v in restated_powerlaw_jackknife(y, r0, r1, ibegin, iend)]
    return max(abs(g - w) / abs(w) for g, w in zip((lnc, q, se_c, se_q), want))       # plain relative, all four


def test_the_fit_against_the_long_double_restatement():
    """normcurve_fitpowerlaw.m through polyfit's normal equations in long double, on 40 seeded arrays of 8 .. 48 points
    whose ranges span more than a decade, 2 .. 12 batches of lognormal scatter.  Observed on the CPU over these seeds: the
    worst relative deviation of (ln c, q, se(ln c), se(q)) is 2.2e-14, so 100 times it is 2.2e-12 -- asserted: that, and
    never looser than 1e-10."""
    worst = max(fit_deviation(seed) for seed in FIT_SEEDS)
    print(f"fit: worst relative deviation from the long-double restatement over {len(FIT_SEEDS)} seeds = {worst:.3g}")
    assert worst <= min(FIT_TOLERANCE, 100 * 2.2e-14)


def test_the_fit_recovers_an_exact_power_law_and_its_total_is_the_batches_sum():
    X = 10.0 + np.arange(12) * (190.0 / 11)
    rc, lnc, q = host_powerlaw(2.5 * X ** -1.75, 10.0, 200.0, 3, 12)
    assert rc == 0 and lnc == pytest.approx(math.log(2.5), rel=1e-12) and q == pytest.approx(-1.75, rel=1e-12)
    y = np.stack([0.25 * 2.5 * X ** -1.75] * 4)
    rc, lnc, q, se_c, se_q, total = host_powerlaw(y, 10.0, 200.0, 1, 12)
    assert rc == 0 and (total == ((y[0] + y[1]) + y[2]) + y[3]).all()
    assert q == pytest.approx(-1.75, rel=1e-12) and se_c == 0.0 and se_q == 0.0      # equal batches: no spread


def test_the_fits_nan_rules_and_refusals():
    X = 10.0 + np.arange(10) * 10.0
    Y = 3.0 * X ** -2.0
    for bad in (0.0, -1.0, math.nan):
        Z = Y.copy()
        Z[4] = bad
        rc, lnc, q = host_powerlaw(Z, 10.0, 100.0, 2, 9)
        assert rc == 0 and math.isnan(lnc) and math.isnan(q)
        rc, lnc, q = host_powerlaw(Z, 10.0, 100.0, 6, 10)                    # outside the range: no matter
        assert rc == 0 and q == pytest.approx(-2.0, rel=1e-12)
    # the jackknife: one batch holds all of a receiver's energy -> that leave-one-out Y is zero -> se NaN, the fit stands
    y = np.stack([Y / 3] * 3)
    y[0, 5], y[1, 5], y[2, 5] = Y[5], 0.0, 0.0
    rc, lnc, q, se_c, se_q, _ = host_powerlaw(y, 10.0, 100.0, 1, 10)
    assert rc == 0 and q == pytest.approx(-2.0, rel=1e-12) and math.isnan(se_c) and math.isnan(se_q)
    rc, lnc, q, se_c, se_q, _ = host_powerlaw(y[:1], 10.0, 100.0, 1, 10)      # B = 1: a fit without an error
    assert rc == 0 and not math.isnan(q) and math.isnan(se_c) and math.isnan(se_q)
    # refused, nothing written: A < 2, fewer than 2 points, a range outside the array
    for A, ibegin, iend in ((1, 1, 1), (10, 4, 4), (10, 5, 4), (10, 0, 5), (10, 3, 11)):
        rc, lnc, q = host_powerlaw(Y[:A], 10.0, 100.0, ibegin, iend)
        assert rc != 0 and lnc == -7.0 and q == -7.0, (A, ibegin, iend)
        rc, lnc, q, se_c, se_q, total = host_powerlaw(y[:, :A], 10.0, 100.0, ibegin, iend)
        assert rc != 0 and lnc == -7.0 and se_q == -7.0 and (total == -7.0).all()


def test_the_library_wraps_the_same_fit():
    from radiative3d_amd import array_powerlaw
    A, r0, r1, y, ibegin, iend = fit_case(3)
    rc, lnc, q, se_c, se_q, total = host_powerlaw(y, r0, r1, ibegin, iend)
    got = array_powerlaw(y, r0, r1, ibegin, iend)
    assert got[:4] == pytest.approx((lnc, q, se_c, se_q), rel=1e-12) and np.allclose(got[4], total, rtol=1e-15)
    assert array_powerlaw(total, r0, r1, ibegin, iend) == pytest.approx((lnc, q), rel=1e-12)
    with pytest.raises(RuntimeError, match="at least 2"):
        array_powerlaw(total[:1], r0, r1, 1, 1)
