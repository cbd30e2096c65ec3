"""The envelope misfit against observed data with jackknife errors on the GPU: the kernel (r3d_envelope_misfit) against the host
build of the lines it runs, bit for bit; the known answers on the device; against r3d_envelope_shape where they compute the
same thing; the run that does all of it where the blocks lie (r3d_run_batched_envelope_misfit); and ./main --envelope-fit end
to end."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest
import torch

from array_image_cases import WEIGHTS
from misfit_cases import (BATCHES, CHI, DC, DPK, F64, FIRST, LAG, LAGS, LDS_BINS, LENGTHS, N_BINS, NAN_BITS, ONLY_X, RHO, S_, SMOOTH,
                          STARTS, bits, bounds, host_envelope_misfit, noisy_blocks, observed_rows, planted_blocks, rows_as_blocks,
                          same_bits, write_observed)
from cli_support import main_exe
from octave_text import read_octave
from radiative3d_amd import Engine, Model, _ffi, envelope_misfit, envelope_shape
from radiative3d_amd.model import misfit_spec
from tests.configs import halfspace

pytestmark = pytest.mark.gpu

GUARD = 64
COUNTS = ("bad", "bad_observed")


def run_kernel(x, windows, observed, first, last, weights, ms, mo, lag, amp, ask=F64 + ("lit",) + COUNTS):
    """r3d_envelope_misfit into guarded outputs, twice: the outputs as numpy, after the checks that belong to every launch --
    the second run has the first one's bits, the blocks, the bins and the observed rows are unchanged, the guards behind
    every output stand, an output that was not asked for (not in `ask`, or an se with B < 2) is untouched."""
    L = _ffi.hip_lib()
    B, S, n_bins = x.shape[:3]
    A = last - first + 1
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dbins = torch.from_numpy(np.ascontiguousarray(windows, dtype=np.uint32).view(np.int32).reshape(A, 2)).cuda()
    dobs = torch.from_numpy(np.ascontiguousarray(observed, dtype=np.float64).reshape(A, n_bins)).cuda()
    keep, keep_bins, keep_obs = dx.clone(), dbins.clone(), dobs.clone()
    n_lags = 2 * lag + 1
    sizes = dict(misfit=A * 6, misfit_se=A * 6, xcorr=A * n_lags, xcorr_se=A * n_lags, envelope=A * n_bins, lit=A, bad=1, bad_observed=1)
    asked = {name: name in ask and not (name.endswith("_se") and B < 2) for name in sizes}
    outs = []
    for _ in range(2):
        t = {}
        for name, n in sizes.items():
            if name in F64:
                t[name] = torch.full((n + GUARD,), -7.0, dtype=torch.float64, device="cuda")
            else:
                t[name] = torch.full((n + GUARD,), -7, dtype=torch.int64 if name in COUNTS else torch.int32, device="cuda")
        spec = misfit_spec(S, n_bins, first, last, weights, dbins.data_ptr(), dobs.data_ptr(), ms, mo, lag, amp)
        rc = L.r3d_envelope_misfit(0, B, dx.data_ptr(), C.byref(spec), *[t[name].data_ptr() if asked[name] else None for name in sizes],
                                   torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.r3d_last_error().decode()
        torch.cuda.synchronize()
        got = {}
        for name, n in sizes.items():
            if not asked[name]:
                assert (t[name] == -7).all(), name                  # (not asked for: not touched)
                got[name] = None
                continue
            assert (t[name][n:] == -7).all(), name
            got[name] = t[name][:n].cpu().numpy()
        outs.append(got)
    by_bits = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))     # noqa: E731  (a block may hold NaN)
    assert by_bits(dx, keep) and torch.equal(dbins, keep_bins) and by_bits(dobs, keep_obs)
    for name in sizes:
        if outs[0][name] is not None:
            same = bits(outs[0][name]) == bits(outs[1][name]) if name in F64 else outs[0][name] == outs[1][name]
            assert same.all(), name
    return outs[0]


def check_against_host(x, windows, observed, first, last, weights, ms, mo, lag, amp, what, **kw):
    got = run_kernel(x, windows, observed, first, last, weights, ms, mo, lag, amp, **kw)
    want = host_envelope_misfit(x, windows, observed, first, last, weights, ms, mo, lag, amp)
    try:
        same_bits({k: (None if v is None else (int(v[0]) if k in COUNTS else v)) for k, v in got.items()},
                  {k: (want[k] if got[k] is not None else None) for k in got})
    except AssertionError as e:
        raise AssertionError((what,) + e.args) from None
    return got, want


# ---- the kernel alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", LENGTHS + (136,))                # 136: from bin 64 to the last of the 200
def test_envelope_misfit_kernel_equals_the_host_build_bit_for_bit(length):
    """Every window length around the 64 strands and the kernel's 64-bin tile, starting off the tile boundary, for every B and
    A with a zero row; the smoothing counts on either side, the lags (a tile of four lags at a time: 1, 3, 11 and 129 of them),
    the three weight sets, amplitudes and energies turn over the cases."""
    rng = np.random.default_rng(11000 + length)
    obs = observed_rows(3, N_BINS, rng)
    n = 0
    for B in BATCHES:
        x = planted_blocks(B, N_BINS, rng)
        for A in (1, 3):
            for ms in SMOOTH:
                mo, lag, amp, weights = SMOOTH[(n // 2 + 1) % 4], LAGS[(n + n // 4) % 4], (n // 3) % 2, WEIGHTS[n % 3]
                windows = [[STARTS[(n + i) % 3], STARTS[(n + i) % 3] + length] for i in range(A)]
                n += 1
                got, want = check_against_host(x, windows, obs[:A], FIRST, FIRST + A - 1, weights, ms, mo, lag, amp,
                                               (length, B, A, ms, mo, lag, amp))
                nan = (bits(got["misfit"]) == NAN_BITS).reshape(A, 6)
                if length == 0:
                    assert want["lit"].tolist() == [0] * A and nan.all()
                elif A == 3:
                    assert want["lit"].tolist() == [1, 1, 0] and nan[2].all() and not nan[:2].any()
                    assert (bits(got["envelope"].reshape(3, N_BINS)[2]) == 0).all()                     # the zero row: +0.0


def test_a_window_longer_than_the_rows_the_lag_scan_keeps_in_lds():
    """n_bins = LDS_BINS + 1, the smallest that crosses the limit: receiver 0's window is one bin too long for LDS and goes
    through the scratch, receiver 1's fits exactly."""
    rng = np.random.default_rng(11100)
    n_bins = LDS_BINS + 1
    x = noisy_blocks(2, 3, n_bins, rng)
    obs = observed_rows(2, n_bins, rng)
    for lag in (5, 64):
        got, want = check_against_host(x, [[0, n_bins], [1, n_bins]], obs, 1, 2, WEIGHTS[2], 1, 1, lag, 1, ("lds", lag))
        assert want["lit"].tolist() == [1, 1] and np.isfinite(got["misfit_se"]).all()


def test_dead_rows_bad_observed_values_and_bad_windows():
    rng = np.random.default_rng(11200)
    x = planted_blocks(3, N_BINS, rng)
    obs = observed_rows(3, N_BINS, rng)
    for value in (-1.0, -5e-324, math.inf, math.nan):
        inside = obs.copy()
        inside[0, 70], inside[1, 5], inside[1, 199] = value, value, value            # receiver 1's lie outside its window
        got, _ = check_against_host(x, [[64, 128], [6, 199], [0, N_BINS]], inside, FIRST, FIRST + 2, WEIGHTS[1], 8, 1, 5, 1, ("bad", value))
        assert int(got["bad_observed"][0]) == 1 and got["lit"].tolist() == [0, 1, 0] and int(got["bad"][0]) == 0
    zero_obs = obs.copy()
    zero_obs[1] = 0.0
    got, _ = check_against_host(x, [[1, 131], [1, 131], [70, 70]], zero_obs, FIRST, FIRST + 2, WEIGHTS[0], 1, 8, 64, 0, "zero observed")
    assert got["lit"].tolist() == [1, 0, 0] and int(got["bad_observed"][0]) == 0
    x[:, FIRST + 2] = np.nan                                                         # never read through
    obs[2] = -1.0
    got, _ = check_against_host(x, [[150, N_BINS], [70, 70], [9, 3]], obs, FIRST, FIRST + 2, WEIGHTS[2], 8, 0, 5, 1, "cut, empty, reversed")
    assert int(got["bad"][0]) == 1 and int(got["bad_observed"][0]) == 0 and got["lit"].tolist() == [1, 0, 0]
    got, _ = check_against_host(x, [[0, N_BINS + 1]], obs[2:], FIRST + 2, FIRST + 2, WEIGHTS[2], 8, 0, 5, 1, "past the blocks")
    assert int(got["bad"][0]) == 1 and got["lit"].tolist() == [0]


def test_more_receivers_than_workgroups_of_one_launch():
    """700 receivers: a workgroup serves several of them in turn, through the same scratch rows and the same LDS."""
    rng = np.random.default_rng(11300)
    A, n_bins = 700, 70
    x = rng.lognormal(0.0, 1.0, (3, A + 1, n_bins, 5))
    x[:, 1::7, :40] = 0.0
    x[:, 5::50] = 0.0
    obs = rng.lognormal(0.0, 1.0, (A, n_bins))
    obs[3::40] = 0.0
    obs[11::90, 20] = -2.0
    windows = [[i % 5, n_bins - i % 3] for i in range(A)]
    got, want = check_against_host(x, windows, obs, 1, A, WEIGHTS[2], 3, 2, 5, 1, "700 receivers")
    assert 0 < want["lit"].sum() < A and int(got["bad_observed"][0]) == len(range(11, A, 90))


def test_outputs_that_are_not_asked_for_are_not_touched():
    rng = np.random.default_rng(11400)
    x = planted_blocks(3, N_BINS, rng)
    obs = observed_rows(3, N_BINS, rng)
    windows = [[1, 131], [63, 193], [64, 128]]
    full, _ = check_against_host(x, windows, obs, FIRST, FIRST + 2, WEIGHTS[0], 8, 1, 5, 1, "all")
    for ask in (("misfit",), ("misfit", "xcorr_se"), ("misfit", "misfit_se", "lit"), ("misfit", "xcorr", "envelope", "bad"),
                ("misfit", "bad_observed")):
        got, _ = check_against_host(x, windows, obs, FIRST, FIRST + 2, WEIGHTS[0], 8, 1, 5, 1, ask, ask=ask)
        assert (bits(got["misfit"]) == bits(full["misfit"])).all()


def test_receivers_whose_offset_passes_2_to_31_doubles():
    """[2][S][130][5] with S * 650 > 2^31: the array is the last three receivers, whose bins lie past a 32-bit offset in both
    blocks (and the second block's start does too)."""
    rng = np.random.default_rng(11500)
    n_bins = 130
    S = (1 << 31) // (n_bins * 5) + 7
    tail = planted_blocks(2, n_bins, rng)[:, FIRST:FIRST + 3]
    tail[:, 2] = tail[:, 0][:, ::-1]                                                                     # (no zero row here)
    obs = observed_rows(3, n_bins, rng)
    x = torch.zeros((2, S, n_bins, 5), dtype=torch.float64, device="cuda")
    x[:, S - 3:] = torch.from_numpy(tail).cuda()
    windows = np.array([[1, 130], [0, 65], [64, 129]], dtype=np.int32)
    out = envelope_misfit(x, torch.from_numpy(windows).cuda(), torch.from_numpy(obs).cuda(), S - 3, S - 1, WEIGHTS[2], 8, 1, 5, 1)
    torch.cuda.synchronize()
    want = host_envelope_misfit(tail, windows, obs, 0, 2, WEIGHTS[2], 8, 1, 5, 1)
    same_bits({k: (v.cpu().numpy() if k in F64 + ("lit",) else int(v[0])) for k, v in out.items()}, want)
    assert want["lit"].tolist() == [1, 1, 1]


def test_refusals_enqueue_nothing():
    L = _ffi.hip_lib()
    x = torch.full((2, 5, 40, 5), 1.5, dtype=torch.float64, device="cuda")
    bins = torch.tensor([[0, 40]] * 3, dtype=torch.int32, device="cuda")
    obs = torch.full((3, 40), 2.0, dtype=torch.float64, device="cuda")
    out = {n: torch.full((3 * 40,), -7.0, dtype=torch.float64, device="cuda") for n in ("misfit", "se", "xcorr", "xse", "env")}
    ints = {n: torch.full((8,), -7, dtype=torch.int64, device="cuda") for n in ("lit", "bad", "bad_observed")}

    def call(B=2, blocks=x.data_ptr(), misfit=out["misfit"].data_ptr(), se=out["se"].data_ptr(), xse=out["xse"].data_ptr(),
             spec="spec", **kw):
        s = misfit_spec(5, kw.pop("n_bins", 40), kw.pop("first", 1), kw.pop("last", 3), kw.pop("weights", (1, 1, 1, 0, 0)),
                        kw.pop("bins", bins.data_ptr()), kw.pop("observed", obs.data_ptr()), kw.pop("smooth_syn", 8),
                        kw.pop("smooth_obs", 1), kw.pop("max_lag", 5), kw.pop("amplitude", 1))
        for key, v in kw.items():
            setattr(s, key, v)
        return L.r3d_envelope_misfit(0, B, blocks, C.byref(s) if spec else None, misfit, se, out["xcorr"].data_ptr(), xse,
                                     out["env"].data_ptr(), ints["lit"].data_ptr(), ints["bad"].data_ptr(),
                                     ints["bad_observed"].data_ptr(), None)

    refused = [dict(blocks=None), dict(spec=None), dict(misfit=None), dict(bins=None), dict(observed=None), dict(size=4), dict(B=0),
               dict(B=65), dict(n_bins=0), dict(first=3, last=2), dict(last=5), dict(weights=(1, -1, 1, 0, 0)),
               dict(weights=(math.nan, 1, 1, 0, 0)), dict(smooth_syn=65), dict(smooth_obs=65), dict(max_lag=65), dict(amplitude=2),
               dict(B=1), dict(B=1, se=None)]
    for kw in refused:
        assert call(**dict(kw)) != 0, kw
        assert L.r3d_last_error().decode().startswith("r3d_envelope_misfit: "), kw
    torch.cuda.synchronize()
    assert all((t == -7.0).all() for t in out.values()) and all((t == -7).all() for t in ints.values())
    assert call() == 0 and call(B=1, se=None, xse=None) == 0 and call(smooth_syn=0, max_lag=0) == 0     # and these go through
    torch.cuda.synchronize()
    six = out["misfit"][:18].reshape(3, 6).cpu().numpy()
    assert np.isfinite(six).all() and (six[:, S_] > 0).all()


# ---- known answers on the device ------------------------------------------------------------------------------------------
def test_known_answers_on_the_device():
    """Observed = the call's own envelope: s = 1 exactly, chi, dpk and dc +0.0, lag 0, rho within the header's bound of 1.
    Observed = 3 times a compact row, 5 bins later: lag 5 and c_5 within the bound of 1.  Blocks times 2^20 under amplitude = 1:
    s times 2^10 exactly, the other five and the curve unchanged to the bit."""
    rng = np.random.default_rng(11600)
    B, n_bins, ms, lag = 3, 130, 8, 64
    x = torch.from_numpy(noisy_blocks(B, 4, n_bins, rng)).cuda()
    windows = [[0, n_bins], [3, n_bins - 2], [43, 83]]
    dbins = torch.tensor(windows, dtype=torch.int32, device="cuda")
    first = envelope_misfit(x, dbins, torch.ones((3, n_bins), dtype=torch.float64, device="cuda"), 1, 3, WEIGHTS[2], ms, 0, lag, 1)
    got = envelope_misfit(x, dbins, first["envelope"].clone(), 1, 3, WEIGHTS[2], ms, 0, lag, 1)
    torch.cuda.synchronize()
    six, curve = got["misfit"].cpu().numpy(), got["xcorr"].cpu().numpy()
    for i, (b0, b1) in enumerate(windows):
        assert six[i, S_] == 1.0 and (bits(six[i, [CHI, DPK, DC]]) == 0).all() and six[i, LAG] == 0.0, (i, six[i])
        assert abs(six[i, RHO] - 1.0) <= bounds(B, b1 - b0, ms, 0, 1)["c"] and curve[i, lag] == six[i, RHO]
    assert np.isfinite(got["misfit_se"].cpu().numpy()).all()

    n = 120
    k = np.arange(n, dtype=np.float64)
    row = np.clip(1.0 - np.abs(k - 50.0) / 10.0, 0.0, None) ** 2 * 5.0
    rows = np.zeros((1, 1, n))
    rows[0, 0] = row
    xr = torch.from_numpy(rows_as_blocks(rows)).cuda()
    whole = torch.tensor([[0, n]], dtype=torch.int32, device="cuda")
    u = envelope_misfit(xr, whole, torch.ones((1, n), dtype=torch.float64, device="cuda"), 0, 0, ONLY_X, 0, 0, 0, 1)["envelope"]
    obs = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    obs[0, 5:] = 3.0 * u[0, :-5]
    for lag in (5, 64):
        out = envelope_misfit(xr, whole, obs, 0, 0, ONLY_X, 0, 0, lag, 1)
        torch.cuda.synchronize()
        assert float(out["misfit"][0, LAG]) == 5.0 and abs(float(out["xcorr"][0, lag + 5]) - 1.0) <= bounds(1, n, 0, 0, 1)["c"]

    obs = torch.from_numpy(observed_rows(3, n_bins, rng)).cuda()
    a = envelope_misfit(x, dbins, obs, 1, 3, WEIGHTS[2], ms, 1, 5, 1)
    b = envelope_misfit(x * 2.0 ** 20, dbins, obs, 1, 3, WEIGHTS[2], ms, 1, 5, 1)
    torch.cuda.synchronize()
    a, b = ({k: v.cpu().numpy() for k, v in o.items()} for o in (a, b))
    rest = [RHO, CHI, DPK, LAG, DC]
    assert (b["misfit"][:, S_] == a["misfit"][:, S_] * 2.0 ** 10).all() and (bits(b["misfit"][:, rest]) == bits(a["misfit"][:, rest])).all()
    assert (bits(b["misfit_se"][:, rest]) == bits(a["misfit_se"][:, rest])).all() and (bits(b["xcorr"]) == bits(a["xcorr"])).all()
    assert (bits(b["xcorr_se"]) == bits(a["xcorr_se"])).all()


# ---- consistency with the sibling -----------------------------------------------------------------------------------------
def test_the_envelope_of_energies_is_the_envelope_shapes():
    """amplitude = 0: the rows and the passes are r3d_envelope_shape's, so the returned envelope is its envelope, bit for bit."""
    rng = np.random.default_rng(11700)
    for B, n_bins, m in ((1, 65, 0), (3, 200, 8), (16, 400, 4)):
        x = planted_blocks(B, n_bins, rng)
        x[:, FIRST + 2] = x[:, FIRST][:, ::-1]
        dx = torch.from_numpy(x).cuda()
        dbins = torch.tensor([[1, n_bins], [0, 64], [n_bins // 3, n_bins - 1]], dtype=torch.int32, device="cuda")
        obs = torch.from_numpy(observed_rows(3, n_bins, rng)).cuda()
        for weights in WEIGHTS:
            fit = envelope_misfit(dx, dbins, obs, FIRST, FIRST + 2, weights, m, 1, 5, 0)
            shp = envelope_shape(dx, dbins, FIRST, FIRST + 2, weights, m)
            torch.cuda.synchronize()
            assert torch.equal(fit["envelope"].view(torch.int64), shp["envelope"].view(torch.int64)) and (fit["envelope"] > 0).any()
            assert torch.equal(fit["lit"], shp["lit"])


# ---- the run that does it all ---------------------------------------------------------------------------------------------
AXES = (1.0, 1.0, 1.0, 0.0, 0.0)
N, B_RUN, SEED, MS, MO, LAG_RUN = 8000, 4, 0x5EED, 8, 2, 5


def test_run_batched_envelope_misfit_equals_run_batched_and_the_call_on_its_kept_blocks(models):
    """r3d_run_batched_envelope_misfit against r3d_run_batched of the same histories and the device-level call on the blocks
    that run kept.  Counts and scalars are equal.  Two runs of the same histories agree to summation order and not to the bit (the
    bins are summed by atomic adds; tests/test_envelope_shape_gpu.py has the count), so energies are held to
    tests/test_gpu_parity.energies_agree's figure, 1e-11 of a bin's P + S energy in each component, and the misfit to what
    that figure moves it by: with the weights (1, 1, 1, 0, 0) a bin's weighted energy moves by r = 3e-11 PS_b / t_b of itself at
    most, and so does every value of u (a root halves it, a pass is a convex combination).  s is linear in u: r s.  rho and
    every c_L: 2 r (numerator and norm).  chi and dpk by the header's bounds with r in place of e1 and 2 r in place of e2, e3
    and e4; dc by 2 r cu with cu <= n.  lag is held where the curve's maximum stands 4 r above the rest.  How many entries
    differ in their bits at all is printed."""
    e = Engine(models("halfspace", 3), reproducible=True)
    try:
        m = e.model
        S, n_bins = m.n_seismometers, m.n_bins
        _, bins, _ = m.envshape_plan(dict(first=0, last=S - 1))
        res0, ese0, cse0, be, _ = e.run_batched(N, B_RUN, seed=SEED, keep_batches=True)
        dbe = torch.from_numpy(be).cuda()
        dbins = torch.from_numpy(bins.view(np.int32)).cuda()
        plain = envelope_misfit(dbe, dbins, torch.ones((S, n_bins), dtype=torch.float64, device="cuda"), 0, S - 1, AXES, MS, 0, 0, 1)
        # an observed record per receiver: the run's own envelope, two bins later and half as high
        obs = torch.zeros((S, n_bins), dtype=torch.float64, device="cuda")
        obs[:, 2:] = 0.5 * plain["envelope"][:, :-2]
        for i, (b0, b1) in enumerate(bins):
            obs[i, :b0] = 0.0
        want = {k: v.cpu().numpy() for k, v in envelope_misfit(dbe, dbins, obs, 0, S - 1, AXES, MS, MO, LAG_RUN, 1).items()}
        torch.cuda.synchronize()
        res, ese, cse, fit = e.run_batched_envelope_misfit(N, B_RUN, bins, obs.cpu().numpy(), 0, S - 1, AXES, MS, MO, LAG_RUN, 1, seed=SEED)
    finally:
        e.close()
    from tests.test_gpu_parity import energies_agree
    assert (res.counts == res0.counts).all() and (res.scalars() == res0.scalars()).all()
    ps = be.sum(axis=0)[..., 3:].sum(-1)
    assert energies_agree(res0.energy, res.energy) and np.allclose(cse, cse0, rtol=1e-12, atol=0)
    assert np.allclose(ese, ese0, rtol=1e-6, atol=1e-11 * ps.max())
    t = be.sum(axis=0)[..., :3].sum(-1)
    with np.errstate(all="ignore"):
        r = np.where(t > 0, 3e-11 * ps / t, 0.0).max(axis=1)
    print(f"largest relative move of a bin's weighted energy that the parity figure allows: {r.max():.3g}")
    assert r.max() < 1e-9
    lit = want["lit"].astype(bool)
    assert (fit["lit"] == want["lit"].view(np.uint32)).all() and lit.any() and int(want["bad_observed"][0]) == 0
    six, wsix = fit["misfit"][lit], want["misfit"][lit]
    rl, n_win = r[lit], (bins[lit, 1] - bins[lit, 0]).astype(np.float64)
    assert (np.abs(fit["envelope"] - want["envelope"]) <= r[:, None] * want["envelope"]).all()
    assert (np.abs(six[:, S_] - wsix[:, S_]) <= rl * wsix[:, S_]).all()
    assert (np.abs(six[:, RHO] - wsix[:, RHO]) <= 2 * rl * wsix[:, RHO]).all()
    assert (np.abs(fit["xcorr"][lit] - want["xcorr"][lit]) <= 2 * rl[:, None] * want["xcorr"][lit]).all()
    for q, e1 in ((CHI, rl), (DPK, 2 * rl)):
        root = np.sqrt(wsix[:, q])
        assert (np.abs(six[:, q] - wsix[:, q]) <= 4 * e1 * root + 4 * e1 ** 2 + 2 * rl * (root + 2 * e1) ** 2).all(), q
    assert (np.abs(six[:, DC] - wsix[:, DC]) <= 2 * rl * n_win).all()
    top = np.sort(want["xcorr"][lit], axis=1)
    clear = (top[:, -1] - top[:, -2]) > 4 * rl
    assert clear.any() and (six[clear, LAG] == wsix[clear, LAG]).all() and (wsix[clear, LAG] == 2.0).mean() > 0.5
    off = int((bits(fit["misfit"]) != bits(want["misfit"])).sum() + (bits(fit["misfit_se"]) != bits(want["misfit_se"])).sum())
    print(f"entries of misfit and misfit_se whose bits differ between the run and the call on a second run's blocks: {off} of {2 * fit['misfit'].size}")
    fin = np.isfinite(want["misfit_se"]).all(axis=1) & lit
    assert (np.isfinite(fit["misfit_se"]).all(axis=1) == np.isfinite(want["misfit_se"]).all(axis=1)).all()
    # the errors: a jackknife of B values that each move by `move` moves by sqrt(B) times the largest such move
    f = B_RUN / (B_RUN - 1.0)
    if fin.any():
        for q, move in ((S_, r * np.abs(want["misfit"][:, S_]) * f * 2), (RHO, 4 * r)):
            assert (np.abs(fit["misfit_se"][fin, q] - want["misfit_se"][fin, q]) <= math.sqrt(B_RUN) * 4 * move[fin] + 1e-300).all(), q


# ---- ./main --envelope-fit ---------------------------------------------------------------------------------------------------
def test_cli_envelope_fit_end_to_end(tmp_path):
    """A first run against a flat record leaves the run's own smoothed amplitude envelope in envfit.octv; written out as the
    observed file on the run's own abscissae, a second run of the same histories fits it: lag 0, and -- two runs of the same
    histories agreeing to summation order, 1e-10 of a bin at the most -- s within 1e-9 of 1, rho within 1e-9 of 1 and chi, the
    square of such a difference, below 1e-18.  Both runs write the same traces."""
    args = halfspace(4) + ["--num-phonons=500K", "--seed=77", "--error-batches=8"]
    fit = ["--envelope-fit-array=48,95", "--envelope-fit-axes=1,1,0"]
    model = Model(args)
    n_bins, dt, A = model.n_bins, model.desc.params.time_per_bin, 48
    flat = write_observed(tmp_path / "flat.octv", (0.0, n_bins * dt), np.ones((2, A)))
    own = str(tmp_path / "own.octv")
    runs = (("first", fit + [f"--envelope-fit={flat},3.6,0,-2,60,4,0,2.0"]), ("second", fit + [f"--envelope-fit={own},3.6,0,-2,60,4,0,2.0"]))
    got = {}
    for name, more in runs:
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([main_exe()] + args + [f"--output-dir={out}"] + more, cwd=out, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        got[name] = read_octave(out / "envfit.octv")
        if name == "first":
            write_observed(own, (0.0, n_bins * dt), got["first"]["FitEnvelope"].T)
    names = sorted(p.name for p in (tmp_path / "first").glob("seis_*.octv"))
    assert len(names) == 288 and names == sorted(p.name for p in (tmp_path / "second").glob("seis_*.octv"))
    for name in names[96:100]:                                      # (at the 6 digits of the trace files)
        assert (tmp_path / "first" / name).read_bytes() == (tmp_path / "second" / name).read_bytes(), name
    first, second = got["first"], got["second"]
    assert (second["FitSeismometers"][:, 0] == np.arange(48, 96)).all() and second["FitBatches"] == 8 and second["FitNumBins"] == n_bins
    assert second["FitSmooth"].tolist() == [[4, 0]] and second["FitAxes"].tolist() == [[1, 1, 0]] and second["FitMaxLag"] == round(2.0 / dt)
    plan = Model(args + runs[1][1]).envfit_plan()
    assert (second["FitDistances"][:, 0] == plan[0]).all() and (second["FitBins"] == plan[1]).all()
    assert (bits(second["FitObserved"]) == bits(plan[3])).all()
    # the observed rows ARE the first run's envelope: the record's samples sit on the bins' abscissae
    assert (bits(second["FitObserved"]) == bits(first["FitEnvelope"])).all()
    lit = second["FitLit"][:, 0] == 1
    assert lit.sum() >= 10 and (first["FitLit"][:, 0] == second["FitLit"][:, 0]).all()
    assert (np.abs(second["FitScale"][lit, 0] - 1.0) <= 1e-9).all() and (np.abs(second["FitCorrelation"][lit, 0] - 1.0) <= 1e-9).all()
    assert (second["FitResidual"][lit, 0] <= 1e-18).all() and (second["FitResidual"][lit, 0] >= 0).all()
    assert (second["FitLag"][lit, 0] == 0).all() and (second["FitLagSeconds"][lit, 0] == 0).all()
    assert (np.abs(second["FitCentroidShift"][lit, 0]) <= 1e-7).all() and (second["FitPeakDistance"][lit, 0] <= 1e-18).all()
    assert np.isnan(second["FitScale"][~lit, 0]).all()
    assert np.allclose(second["FitEnvelope"], first["FitEnvelope"], rtol=1e-9, atol=0)
    # against the flat record the scale is the envelope's mean level and the fit is poor
    assert (first["FitScale"][lit, 0] > 0).all() and (first["FitResidual"][lit, 0] > 1e-3).all()
    print(f"{lit.sum()} of {A} receivers lit; largest |s - 1| {np.abs(second['FitScale'][lit, 0] - 1).max():.3g}, largest chi "
          f"{second['FitResidual'][lit, 0].max():.3g}")
