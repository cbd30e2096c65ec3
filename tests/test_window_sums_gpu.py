"""Lapse-window energies with batch errors on the GPU: the window kernel (r3d_window_sums) against the host build of the
lines it runs, value for value; its composition with r3d_batch_moments on the kept blocks of real batched runs; the run
that does all of it where the blocks lie (r3d_run_batched_windows); and ./main --lapse-windows end to end."""
import ctypes as C
import math
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

from batch_cases import sum_in_order
from cli_support import main_exe
from octave_text import read_octave
from radiative3d_amd import Engine, _ffi, batch_moments, window_sums
from radiative3d_amd.model import window_spec
from tests.configs import halfspace
from window_cases import (WEIGHTS, decimation_windows, exact_window_sum, five_windows, host_moments, host_window_sums,
                          random_blocks, rule_bins, window_bound)

pytestmark = pytest.mark.gpu

LAPSE = dict(phase_edge=(3.6, 0.0), windows=(5.0, 20.0, 45.0, 115.0), axes=(0.0, 0.0, 1.0), geospread=2.0,
             ranges=(8.0, 50.0, 150.0))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def run_kernel(x, c, bins, weights, guard=64):
    """window_sums into guarded outputs, twice: (sums, counts, bad) as numpy, after the checks that belong to every
    launch -- the second run has the first one's bits, the blocks are unchanged, the guards behind both outputs stand."""
    B, S, n_bins = x.shape[:3]
    W = bins.shape[1]
    n = B * S * W
    dx, dc = torch.from_numpy(x).cuda(), torch.from_numpy(c.view(np.int64)).cuda()
    keep_x, keep_c = dx.clone(), dc.clone()
    dbins = torch.from_numpy(bins.view(np.int32)).cuda()
    outs = []
    for _ in range(2):
        ge = torch.full((n + guard,), -7.0, dtype=torch.float64, device="cuda")
        gc = torch.full((2 * n + guard,), -7, dtype=torch.int64, device="cuda")
        y, yc, bad = window_sums(dx, dbins, weights, batch_counts=dc, window_energy=ge[:n], window_counts=gc[:2 * n],
                                 count_bad=True)
        torch.cuda.synchronize()
        assert (ge[n:] == -7.0).all() and (gc[2 * n:] == -7).all()
        outs.append((y.cpu().numpy().reshape(B, S, W), yc.cpu().numpy().view(np.uint64).reshape(B, S, W, 2), int(bad.item())))
    assert torch.equal(dx, keep_x) and torch.equal(dc, keep_c)
    assert (bits(outs[0][0]) == bits(outs[1][0])).all() and (outs[0][1] == outs[1][1]).all() and outs[0][2] == outs[1][2]
    return outs[0]


def check_against_host(x, c, bins, weights, what):
    y, yc, bad = run_kernel(x, c, bins, weights)
    want, want_c, want_bad = host_window_sums(x, bins, weights, c)
    assert (bits(y) == bits(want)).all(), what                      # value for value, the sign of a zero included
    assert (yc == want_c).all() and bad == want_bad, what
    return y, yc, bad


# ---- the kernel alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [1, 63, 64, 65, 400])
def test_window_kernel_equals_the_host_build_value_for_value(n_bins):
    rng = np.random.default_rng(4000 + n_bins)
    k = 0
    for S in (1, 3):
        for B in (1, 2, 64):
            x, c = random_blocks(B, S, n_bins, rng)
            bins = five_windows(n_bins, S, rng)
            for weights in WEIGHTS if B == 2 else (WEIGHTS[k % 4],):
                y, yc, bad = check_against_host(x, c, bins, weights, (n_bins, S, B, weights))
                assert bad == 0 and (bits(y[:, :, 0]) == 0).all()        # the empty window: +0.0
                for s in range(S):
                    for w, (begin, end) in enumerate(bins[s]):
                        assert (yc[:, s, w] == c[:, s, begin:end].sum(axis=1, dtype=np.uint64)).all()   # counts are exact
            k += 1


@pytest.mark.parametrize("weights", WEIGHTS)
def test_window_kernel_on_the_decimation_shape(weights):
    """400 bins as 100 windows of 4 (vis/seisplot/decimate.m): four work-items serve a window."""
    rng = np.random.default_rng(4100)
    for S, B in ((1, 1), (3, 2), (3, 64)):
        x, c = random_blocks(B, S, 400, rng)
        bins = decimation_windows(400, S)
        assert bins.shape == (S, 100, 2)
        y, yc, _ = check_against_host(x, c, bins, weights, ("decimation", S, B, weights))
        assert (yc.sum(axis=2) == c.sum(axis=2, dtype=np.uint64)).all()           # the windows tile the trace


def test_window_kernel_serves_long_and_overlapping_windows_with_few_work_items_and_a_bin_past_2_to_31():
    """The geometry follows the SHAPE (n_bins / n_windows), not the windows: many windows per trace get 4 or 16
    work-items each, however long they are.  And one block large enough that a bin's offset passes 2^31 doubles."""
    rng = np.random.default_rng(4200)
    for n_bins, W in ((130, 40), (400, 30)):                                      # 4 and 16 work-items per window
        S, B = 2, 2
        x, c = random_blocks(B, S, n_bins, rng)
        lo = rng.integers(0, n_bins, (S, W))
        hi = np.minimum(lo + rng.integers(0, n_bins, (S, W)), n_bins)
        bins = np.stack([lo, hi], axis=2).astype(np.uint32)
        bins[0, 0] = (0, n_bins)
        check_against_host(x, c, bins, WEIGHTS[3], (n_bins, W))
    # [1][1][n_bins][5] with 5 * n_bins > 2^31: the last bins lie past a 32-bit offset
    n_bins = (1 << 31) // 5 + 1000
    x = torch.zeros((1, 1, n_bins, 5), dtype=torch.float64, device="cuda")
    tail = rng.lognormal(0.0, 1.0, (700, 5))
    x[0, 0, n_bins - 700:] = torch.from_numpy(tail).cuda()
    bins = np.array([[[n_bins - 700, n_bins], [n_bins - 1, n_bins], [0, 64]]], dtype=np.uint32)
    y, _, _ = window_sums(x, torch.from_numpy(bins.view(np.int32)).cuda(), WEIGHTS[1])
    want, _, _ = host_window_sums(tail[None, None], np.array([[[0, 700], [699, 700], [0, 0]]], dtype=np.uint32), WEIGHTS[1])
    assert (bits(y.cpu().numpy()) == bits(want)).all() and want[0, 0, 0] > 0


def test_a_bad_bin_pair_is_counted_and_adds_nothing():
    rng = np.random.default_rng(4300)
    n_bins, S, B = 130, 3, 2
    x, c = random_blocks(B, S, n_bins, rng)
    bins = five_windows(n_bins, S, rng)
    bins[1, 2] = (90, 20)                                          # begin > end
    bins[2, 3] = (100, n_bins + 1)                                 # end one past the trace
    bins[2, 4] = (0xFFFFFFF0, 0xFFFFFFFF)                          # far outside: never read through
    y, yc, bad = check_against_host(x, c, bins, WEIGHTS[1], "bad pairs")
    assert bad == 3
    for s, w in ((1, 2), (2, 3), (2, 4)):
        assert (bits(y[:, s, w]) == 0).all() and not yc[:, s, w].any()
    # without the counter and without counts the same sums
    y2, none, nobad = window_sums(torch.from_numpy(x).cuda(), torch.from_numpy(bins.view(np.int32)).cuda(), WEIGHTS[1])
    assert none is None and nobad is None and (bits(y2.cpu().numpy()) == bits(y)).all()


def test_refusals_enqueue_nothing():
    L = _ffi.hip_lib()
    x = torch.full((2, 3, 40, 5), 1.5, dtype=torch.float64, device="cuda")
    bins = torch.zeros((3, 2, 2), dtype=torch.int32, device="cuda")
    out = torch.full((2, 3, 2), -7.0, dtype=torch.float64, device="cuda")
    outc = torch.full((2, 3, 2, 2), -7, dtype=torch.int64, device="cuda")
    for kw in (dict(weights=(0, math.nan, 1, 0, 0)), dict(W=0), dict(size=4)):
        spec = window_spec(3, 40, kw.pop("W", 2), bins.data_ptr(), kw.pop("weights", (0, 0, 1, 0, 0)))
        for k, v in kw.items():
            setattr(spec, k, v)
        assert L.r3d_window_sums(0, 2, x.data_ptr(), None, C.byref(spec), out.data_ptr(), None, None, None) != 0
    spec = window_spec(3, 40, 2, bins.data_ptr(), (0, 0, 1, 0, 0))
    assert L.r3d_window_sums(0, 2, x.data_ptr(), None, C.byref(spec), out.data_ptr(), outc.data_ptr(), None, None) != 0
    assert "count blocks" in L.r3d_last_error().decode()
    assert L.r3d_window_sums(0, 0, x.data_ptr(), None, C.byref(spec), out.data_ptr(), None, None, None) != 0
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (outc == -7).all()


# ---- composition on real blocks, and the run that does it all -------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(models):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Engine(models(name, 4))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def composed(engines):
    """name -> the kept blocks of one batched run, the lapse windows of every receiver, and what window_sums +
    batch_moments make of them on the device: computed once, shared, left unchanged."""
    cache = {}

    def get(name, n, B=10, seed=0x5EED):
        if name not in cache:
            e = engines(name)
            m = e.model
            request = dict(LAPSE, first=0, last=m.n_seismometers - 1)
            dist, bins, clipped = m.lapse_plan(request)
            weights = LAPSE["axes"] + (0.0, 0.0)
            res, ese, cse, be, bc = e.run_batched(n, B, seed=seed, keep_batches=True)
            dbe, dbc = torch.from_numpy(be).cuda(), torch.from_numpy(bc.view(np.int64)).cuda()
            dbins = torch.from_numpy(bins.view(np.int32)).cuda()
            y, yc, bad = window_sums(dbe, dbins, weights, batch_counts=dbc, count_bad=True)
            T, Tc, _, se, _ = batch_moments(y, yc)
            torch.cuda.synchronize()
            assert torch.equal(dbe, torch.from_numpy(be).cuda()) and int(bad.item()) == 0
            cache[name] = dict(n=n, B=B, seed=seed, bins=bins, dist=dist, clipped=clipped, weights=weights, res=res, be=be,
                               bc=bc, y=y.cpu().numpy(), yc=yc.cpu().numpy().view(np.uint64), T=T.cpu().numpy(),
                               Tc=Tc.cpu().numpy().view(np.uint64), se=se.cpu().numpy())
        return cache[name]
    return get


CASES = [("halfspace", 50000), ("crustpinch", 20000)]


@pytest.mark.parametrize("name,n", CASES)
def test_window_sums_then_moments_on_the_blocks_of_a_real_run(composed, name, n):
    k = composed(name, n)
    B, bins, be, weights = k["B"], k["bins"], k["be"], k["weights"]
    S = bins.shape[0]
    # Y, T and se: the host build of the two headers on the downloaded blocks, to the bit
    want_y, want_yc, _ = host_window_sums(be, bins, weights, k["bc"])
    assert (bits(k["y"]) == bits(want_y)).all() and (k["yc"] == want_yc).all()
    want_T, want_se = host_moments(want_y)
    assert (bits(k["T"]) == bits(want_T)).all() and (bits(k["se"]) == bits(want_se)).all()
    assert (k["T"] == sum_in_order(k["y"])).all()
    # T against the exact rational sum of the blocks' bins: d + B - 1 roundings on a term's way
    lit = np.flatnonzero(k["T"].reshape(S, 2).any(axis=1))
    assert len(lit) > 0, name                                      # (receivers with energy in a window: the check is not empty)
    worst = 0.0
    for s in lit[:: max(1, len(lit) // 12)]:
        for w in range(2):
            begin, end = (int(v) for v in bins[s, w])
            exact, mag = Fraction(0), Fraction(0)
            for j in range(B):
                t, a = exact_window_sum(be[j, s], begin, end, weights)
                exact, mag = exact + t, mag + a
            lim = window_bound(end - begin, mag, extra=B - 1)
            err = abs(Fraction(float(k["T"][s, w])) - exact)
            assert err <= lim, (name, s, w, float(err), lim)
            if lim > 0:
                worst = max(worst, float(err) / lim)
    print(f"{name}: worst window-total error / bound = {worst:.3f}")
    # window counts: the result's counts summed over the window's bins, exactly
    for s in range(S):
        for w in range(2):
            begin, end = bins[s, w]
            assert (k["Tc"][s, w] == k["res"].counts[s, begin:end].sum(axis=0, dtype=np.uint64)).all()
    assert k["Tc"].sum() > 0 and (k["se"][k["T"] > 0] > 0).all() and (k["se"][k["T"] == 0] == 0).all()


@pytest.mark.parametrize("name,n", CASES)
def test_run_batched_windows_equals_the_composition(engines, composed, name, n):
    k = composed(name, n)
    e = engines(name)
    res, ese, cse, we, wc, wse, bwe = e.run_batched_windows(n, k["B"], k["bins"], k["weights"], seed=k["seed"],
                                                            keep_batch_windows=True)
    assert (res.counts == k["res"].counts).all() and (res.scalars() == k["res"].scalars()).all()
    assert (wc == k["Tc"]).all()
    # energies to the project's engine-against-engine figure: 1e-11 of the P + S energy, here summed over the window, times
    # max |w| (two runs of the same histories on other streams: tests/test_gpu_parity.energies_agree)
    ps = k["res"].energy[..., 3:].sum(-1)
    scale = np.array([[ps[s, b0:b1].sum() for b0, b1 in k["bins"][s]] for s in range(len(ps))]) * max(abs(v) for v in k["weights"])
    assert (np.abs(we - k["T"]) <= 1e-11 * scale + 1e-300).all()
    batch_scale = np.array([[[k["be"][j, s, b0:b1, 3:].sum() for b0, b1 in k["bins"][s]] for s in range(len(ps))]
                            for j in range(k["B"])]) * max(abs(v) for v in k["weights"])
    assert (np.abs(bwe - k["y"]) <= 1e-11 * batch_scale + 1e-300).all()
    assert (we == sum_in_order(bwe)).all() and (bits(wse) == bits(host_moments(bwe)[1])).all()
    assert np.allclose(wse, k["se"], rtol=1e-6, atol=1e-11 * scale.max())
    # ... and the run's own results are r3d_run_batched's
    plain, pese, pcse = e.run_batched(n, k["B"], seed=k["seed"])
    assert (plain.counts == res.counts).all() and np.allclose(pcse, cse, rtol=1e-12, atol=0)
    from tests.test_gpu_parity import energies_agree
    assert energies_agree(plain.energy, res.energy) and np.allclose(pese, ese, rtol=1e-6, atol=1e-11 * ps.max())


def test_run_batched_windows_shares_the_batched_runs_refusals_and_touches_nothing(engines):
    e = engines("crustpinch")
    m = e.model
    L = e._lib
    S, n_bins = m.n_seismometers, m.n_bins
    bins = np.zeros((S, 2, 2), dtype=np.uint32)
    bins[:, 0], bins[:, 1] = (3, 20), (40, 100)
    B = 4

    def fresh():
        res = m.new_result()
        res.energy[:], res.counts[:] = 3.5, 7
        return dict(res=res, ese=np.full(res.energy.shape, -1.0), cse=np.full(res.counts.shape, -1.0),
                    we=np.full((S, 2), 2.5), wc=np.full((S, 2, 2), 5, dtype=np.uint64), wse=np.full((S, 2), -1.0),
                    bwe=np.full((B, S, 2), -2.0))

    def call(n, batches, bufs, the_bins=bins, **spec_kw):
        spec = window_spec(S, n_bins, 2, the_bins.ctypes.data, (0, 0, 1, 0, 0))
        for key, v in spec_kw.items():
            setattr(spec, key, v)
        c = bufs["res"]._as_c()
        rc = L.r3d_run_batched_windows(e._e, n, 0, 0x5EED, batches, C.byref(c), bufs["ese"].ctypes.data_as(_ffi._dp),
                                       bufs["cse"].ctypes.data_as(_ffi._dp), C.byref(spec), bufs["we"].ctypes.data_as(_ffi._dp),
                                       bufs["wc"].ctypes.data_as(C.POINTER(C.c_uint64)), bufs["wse"].ctypes.data_as(_ffi._dp),
                                       bufs["bwe"].ctypes.data_as(_ffi._dp))
        bufs["res"]._from_c(c)
        return rc

    def refused(n, batches, match, **kw):
        bufs = fresh()
        assert call(n, batches, bufs, **kw) != 0 and match in L.r3d_last_error().decode(), L.r3d_last_error().decode()
        r = bufs["res"]
        assert (r.energy == 3.5).all() and (r.counts == 7).all() and not r.scalars().any()
        assert (bufs["ese"] == -1.0).all() and (bufs["cse"] == -1.0).all() and (bufs["we"] == 2.5).all()
        assert (bufs["wc"] == 5).all() and (bufs["wse"] == -1.0).all() and (bufs["bwe"] == -2.0).all()

    refused(1000, 1, "at least 2 batches")
    refused(1000, 65, "at most 64 batches")
    refused(3, 4, "fewer histories")
    from radiative3d_amd.parallel import DeviceResult
    chain = DeviceResult(m, "cuda:0")
    e.run_device(500, 0, 0x5EED, *chain.pointers(), carry="carry")
    torch.cuda.synchronize()
    refused(1000, B, "carried over")
    e.run_device(0, 0, 0x5EED, *chain.pointers(), carry="final")
    torch.cuda.synchronize()
    e.set_event_log(capacity=1 << 12)
    refused(1000, B, "event log")
    e.set_event_log(mask=0, capacity=0)
    e.set_production_finals(0, 1000)
    refused(1000, B, "production-finals")
    e.set_production_finals(0, 0)
    # the spec: the bins are on the host here, so a bad pair is refused, not counted
    worse = bins.copy()
    worse[5, 1] = (40, n_bins + 1)
    refused(1000, B, "window 1 of seismometer 5", the_bins=worse)
    refused(1000, B, "not the model's", n_bins=n_bins - 1)
    refused(1000, B, "is not finite", weight=(C.c_double * 5)(0, 0, math.inf, 0, 0))
    with pytest.raises(RuntimeError, match="at least 2 batches"):
        e.run_batched_windows(1000, 1, bins, (0, 0, 1, 0, 0))
    # with all of that gone the same call goes through: totals ADDED, se and the batches' sums WRITTEN
    bufs = fresh()
    assert call(4000, B, bufs) == 0, L.r3d_last_error().decode()
    plain = e.run(4000)
    assert (bufs["res"].counts - 7 == plain.counts).all()
    want_wc = np.array([[plain.counts[s, b0:b1].sum(axis=0) for b0, b1 in bins[s]] for s in range(S)], dtype=np.uint64)
    assert (bufs["wc"] - 5 == want_wc).all() and want_wc.sum() > 0
    assert (bufs["wse"] >= 0).all() and (bufs["bwe"] >= 0).all()
    assert np.allclose(bufs["we"] - 2.5, sum_in_order(bufs["bwe"]), rtol=1e-12, atol=1e-12)


# ---- ./main --lapse-windows --------------------------------------------------------------------------------------------------
def test_cli_lapse_windows_end_to_end(tmp_path):
    # (2M histories are milliseconds of GPU time and give most receivers of the line a few catches in either window)
    args = halfspace(4) + ["--num-phonons=2M", "--seed=77", "--error-batches=8"]
    plain, lapse = tmp_path / "plain", tmp_path / "lapse"
    plain.mkdir(), lapse.mkdir()
    for out, extra in ((plain, []), (lapse, ["--lapse-windows", "--lapse-array=48,95"])):
        r = subprocess.run([main_exe()] + args + [f"--output-dir={out}"] + extra, cwd=out, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert not (plain / "lapse.octv").exists()
    # the seis and err files are what they are without the lapse options, byte for byte
    names = sorted(p.name for p in plain.glob("seis_*.octv"))
    assert len(names) == 288 and names == sorted(p.name for p in lapse.glob("seis_*.octv"))
    for name in names:
        assert (plain / name).read_bytes() == (lapse / name).read_bytes(), name
    got = read_octave(lapse / "lapse.octv")
    S, dt = 48, 0.5
    assert (got["LapseSeismometers"][:, 0] == np.arange(48, 96)).all() and got["LapseBatches"] == 8
    dist = got["LapseDistances"][:, 0]
    bins = got["LapseBins"].reshape(S, 2, 2).astype(np.int64)
    for w, (o, e) in enumerate(((5.0, 20.0), (45.0, 115.0))):
        begin, end, clipped = rule_bins(dt, 400, dist, 3.6, 0.0, o, e)
        assert (bins[:, w, 0] == begin).all() and (bins[:, w, 1] == end).all() and (got["LapseClipped"][:, w] == clipped).all()
    assert (got["LapseTimes"] == got["LapseBins"] * dt).all()
    E, counts = got["LapseE"], got["LapseCounts"].reshape(S, 2, 2)
    axes = np.array([0.0, 0.0, 1.0])
    for i in range(S):
        seis = read_octave(lapse / f"seis_{48 + i:03d}.octv")
        # range_km.m on the file's own (6-digit) triples
        assert abs(dist[i] - np.hypot(*(seis["Location"][0, :2] - seis["EventLoc"][0, :2]))) <= 1e-5 * max(dist[i], 1.0)
        for w in range(2):
            b0, b1 = bins[i, w]
            # the files carry 6 significant digits, and the terms are non-negative under the default axes
            assert E[i, w] == pytest.approx((seis["TraceXYZ"][b0:b1] @ axes).sum() * dt, rel=1e-5, abs=0)
            assert (counts[i, w] == seis["CountPS"][b0:b1].sum(axis=0)).all()
    # (non-negative batch values: a total's standard error is positive where the total is, and never exceeds it)
    assert (E > 0).any() and (got["LapseE_se"][E > 0] > 0).all() and (got["LapseE_se"] <= E * (1 + 1e-12)).all()
    spread = np.array([math.pow(d, 2.0) for d in dist])[:, None]
    assert (got["LapseRE"] == E * spread).all()
    r1, r1se = got["LapseR1"][:, 0], got["LapseR1_se"][:, 0]
    both = (E[:, 0] > 0) & (E[:, 1] > 0)
    print(f"receivers with energy in window 1 / 2 / both: {(E[:, 0] > 0).sum()} / {(E[:, 1] > 0).sum()} / {both.sum()} of {S}; "
          f"with a jackknife error: {(~np.isnan(r1se)).sum()}")
    assert both.any() and np.isnan(r1[~both]).all() and np.isnan(r1se[~both]).all()
    assert all(r1[i] == math.log10(E[i, 0] / E[i, 1]) for i in np.flatnonzero(both))
    assert (r1se[~np.isnan(r1se)] > 0).all() and (~np.isnan(r1se)).any()
    ref = [int(np.argmin(np.abs(dist - km))) for km in (8, 50, 150)]
    assert got["LapseRefIndex"].tolist() == [ref]
    RE = got["LapseRE"]
    if RE[ref[1], 0] > 0 and RE[ref[2], 0] > 0:
        assert got["LapseR2"][0, 0] == math.log10(RE[ref[1], 0] / RE[ref[2], 0])
    else:
        assert math.isnan(got["LapseR2"][0, 0])
