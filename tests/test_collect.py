"""The receiver collection on the host against a brute-force reference, arrival by arrival.

`build_seis_grid` (r3d_pack.h) plus `collect<0>()` (r3d_step.h) -- the text the kernels run per lane, built by g++
(tests/collect_cases.py HOST_SOURCE) -- over the receiver sets and arrival tables of tests/collect_cases.py, against that
module's long-double reference, which has no grid and tests every receiver on every arrival.  Counts and catches are
equal EXACTLY, no row left out: the random rows keep MARGIN from every decision by the reference's own judgement, the
planted rows sit ON the decisions with arithmetic that is exact in fp64.  tests/test_collect_device.py runs the same
cases through the wave-cooperative code on the device.
"""
import numpy as np
import pytest

import collect_cases as K
from test_rt_solve import MARGIN, TOL


def host(name):
    c = K.case(name)
    return c, K.host_collect(c.seis, c.time_per_bin, c.n_bins, c.arrivals)


@pytest.mark.parametrize("name", K.CASES)
def test_host_collection_equals_the_reference(name):
    c, h = host(name)
    assert c.redraws < 0.01 * c.draws
    assert np.array_equal(h["counts"], c.ref.counts)
    assert np.array_equal(h["catches"], c.ref.catches)
    ok, dev = K.energies_within(h["energy"], c.ref.energy, TOL)
    print(f"\n[collect] {name}: {c.arrivals.shape[0]} arrivals x {c.seis.shape[0]} receivers, {int(c.ref.catches.sum())} catches in "
          f"{int((c.ref.counts.sum(-1) > 0).sum())} bins, {c.redraws} of {c.draws} rows drawn again; energy deviation host {dev:.3g}")
    assert ok, dev
    assert c.ref.catches.sum() > 0.2 * c.arrivals.shape[0]          # (the table is about catches)
    empty = c.ref.counts.sum(-1) == 0
    assert np.all(h["energy"][empty] == 0.0)


def test_the_margin_and_the_redraw_share():
    """Every random row is at least MARGIN from every decision; far fewer than 1 % were drawn again."""
    draws = redraws = 0
    for name in K.CASES:
        c = K.case(name)
        d = np.minimum(c.ref.d_space, c.ref.d_time)
        random_rows = np.setdiff1d(np.arange(c.arrivals.shape[0]), list(c.planted))
        assert d[random_rows].min() >= MARGIN
        draws, redraws = draws + c.draws, redraws + c.redraws
    assert redraws < 0.01 * draws


@pytest.mark.parametrize("name", [n for n in K.CASES if n != "one-hot"])
def test_planted_rows_are_decided_on_the_boundary(name):
    """The reference and the host build take each planted row in the bin worked out by hand, and the rows ARE on their
    decisions: dist == r_out, dist == r_in, t on a bin edge, arv == n_bins bins."""
    c, _ = host(name)
    assert len(c.planted) == K.N_PLANTED[bool(c.seis[0, 3] > 0)]
    assert [int(c.ref.pair_bin[row, 0]) for row in c.planted] == list(c.planted.values())
    d0 = np.minimum(c.ref.d_space, c.ref.d_time)[list(c.planted), 0]
    assert (d0 == 0).sum() >= len(c.planted) - 3          # (all but the correction row and the two pole rows)
    # each planted row alone: receiver 0's counts are the hand-made ones in the host build
    for row, b in c.planted.items():
        one = K.host_collect(c.seis[:1], c.time_per_bin, c.n_bins, c.arrivals[row:row + 1])
        typ = int(c.arrivals[row, 8])
        want = np.zeros((c.n_bins, 2), dtype=np.uint64)
        if b >= 0:
            want[b, typ] = 1
        assert np.array_equal(one["counts"][0], want), (row, b)
    pole = [row for row in c.planted if abs(c.arrivals[row, 5]) == 1 and c.arrivals[row, 8] == 1]
    assert len(pole) == 2 and all(c.ref.pair_bin[row, 0] >= 0 for row in pole)
    wave = slice(64 * (pole[0] // 64), 64 * (pole[0] // 64) + 64)
    oblique = (c.arrivals[wave, 8] == 1) & (np.abs(c.arrivals[wave, 5]) < 1) & (c.ref.catches[wave] > 0)
    assert oblique.sum() >= 5                                 # (S catches of oblique rays share the pole rays' wave)


def test_the_tables_show_the_patterns():
    """The lane patterns the dealing of pairs has to be seen under, from the candidates the engine's own grid returns; the
    hot table's two bins; the spread table's more than 300."""
    c, h = host("crowd-patterns")
    seen = K.lane_patterns(c.seis, c.arrivals, h["candidates"])
    assert all(seen.values()), [k for k, v in seen.items() if not v]
    assert h["candidates"].max() == K.CROWD_SMALL + K.CROWD_LARGE > 128
    hot = K.case("one-hot")
    assert hot.arrivals.shape[0] > 400 and np.all(hot.ref.catches == 1)
    assert sorted(np.nonzero(hot.ref.counts.sum(-1)[0])[0]) == [1, 2]
    spread = K.case("annuli-spread")
    assert (spread.ref.counts.sum(-1) > 0).sum() > 300
    both = spread.seis[:, 3:5]
    assert ((both[:, 0] > 0) != (both[:, 1] > 0)).sum() == 20     # half are annuli for one type only


def test_the_grids_are_the_ones_meant():
    """(b) the cell edge was grown by the loop and the grid stays at or below 4e6 cells; (e) the large sphere covers
    thousands of cells; which item lists fit in LDS beside 256 accumulators is as the cases declare."""
    for name in K.CASES:
        c, h = host(name)
        dim, n_cells, n_items = h["grid"][:3], int(h["grid"][3]), int(h["grid"][4])
        assert n_cells == dim.prod() <= 4e6 and n_items <= 8e6
        assert (K.lds_bytes(n_items) < K.LDS_LIMIT) == c.lds_fits, (name, n_items)
        rad = c.seis[:, 5:7].max(1)
        lo = (c.seis[:, 0:3] - rad[:, None]).min(0)
        hi = (c.seis[:, 0:3] + rad[:, None]).max(0)
        ungrown = np.ceil((hi - lo) / (0.25 * np.sort(rad)[rad.size // 2])) + 1
        if name == "isolated-mixed":
            assert np.all(dim < ungrown / 10) and n_cells > 1e6
        if name == "radii-mixed":
            assert rad.max() == 100 * rad.min() and n_items > 5e5
        if name in ("one-mixed", "annuli-spread"):
            assert np.array_equal(dim, ungrown)


@pytest.mark.parametrize("name", ["one-mixed", "isolated-mixed", "crowd-patterns", "annuli-spread", "radii-mixed"])
def test_a_cell_lists_every_receiver_that_can_catch_in_it(name):
    """The superset property: for points in and around the box, on the spheres' rims and at their six extreme points, the
    items of the point's cell contain every receiver whose larger gather sphere holds the point."""
    c = K.case(name)
    rng = np.random.default_rng(77)
    rad = c.seis[:, 5:7].max(1)
    lo, hi = (c.seis[:, 0:3] - rad[:, None]).min(0), (c.seis[:, 0:3] + rad[:, None]).max(0)
    n = 4000
    s = rng.integers(0, c.seis.shape[0], n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rim = c.seis[s, 0:3] + u * (rad[s] * rng.uniform(0.97, 1.0, n))[:, None]
    inner = c.seis[s, 0:3] + u * (rad[s] * rng.uniform(0.0, 1.0, n))[:, None]
    box = lo - 0.1 * (hi - lo) + rng.uniform(0, 1, (n, 3)) * 1.2 * (hi - lo)
    poles = []
    for k in range(3):
        for sign in (-1.0, 1.0):
            p = c.seis[:, 0:3].copy()
            p[:, k] += sign * rad * (1 - 1e-7)
            poles.append(p)
    points = np.concatenate([rim, inner, box] + poles)
    listed = K.host_collect(c.seis, c.time_per_bin, c.n_bins, points=points)["in_cell"].astype(bool)
    to = c.seis[None, :, 0:3].astype(K.L) - points[:, None, :].astype(K.L)
    holds = np.sqrt((to * to).sum(-1)) <= rad.astype(K.L)[None, :]
    assert holds.sum() > n
    assert not np.any(holds & ~listed), np.argwhere(holds & ~listed)[:5]
