"""Bootstrap percentile bands of the envelope and its six numbers on the GPU: the kernels (r3d_bootstrap_counts_device,
r3d_envelope_bands) against the host build of the lines they run, bit for bit; against r3d_envelope_shape where both compute the
same thing; on the kept blocks of a real batched run; and the run that does all of it where the blocks lie
(r3d_run_batched_envelope_bands)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from array_image_cases import WEIGHTS
from bands_cases import F64, host_envelope_bands, planted_batches
from envelope_cases import CEN, E_, FIRST, N_BINS, NAN_BITS, ONLY_X, P_, STARTS, TP, TQ, WID, bits, planted_blocks, rows_as_blocks
from radiative3d_amd import Engine, _ffi, bootstrap_counts, envelope_bands, envelope_shape
from radiative3d_amd.model import bands_spec

pytestmark = pytest.mark.gpu

GUARD = 64
NAMES = F64 + ("defined", "bad")
LENGTHS = (0, 1, 2, 63, 64, 65, 130, 136)          # around the kernel's 64-bin tile; 136: from bin 64 to the last of the 200
BATCHES = (2, 3, 64)
REPLICATES = (1, 2, 63, 64, 65, 257)               # around the powers of two the columns are padded to; 257: 8 columns at a time
SMOOTH = (0, 1, 8)


def run_kernel(x, windows, first, last, weights, m, R, T, seed, ask=NAMES):
    """r3d_envelope_bands into guarded outputs, twice: the outputs as numpy, after the checks that belong to every launch -- the
    second run has the first one's bits, the blocks and the bins are unchanged, the guards behind every output stand, an output
    that was not asked for is untouched."""
    L = _ffi.hip_lib()
    B, S, n_bins = x.shape[:3]
    A = last - first + 1
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dbins = torch.from_numpy(np.ascontiguousarray(windows, dtype=np.uint32).view(np.int32).reshape(A, 2)).cuda()
    keep, keep_bins = dx.clone(), dbins.clone()
    sizes = dict(envelope=A * n_bins, envelope_lo=A * n_bins, envelope_hi=A * n_bins, shape=A * 6, shape_lo=A * 6, shape_hi=A * 6,
                 defined=A * 6, bad=1)
    outs = []
    for _ in range(2):
        t = {}
        for name, n in sizes.items():
            if name in F64:
                t[name] = torch.full((n + GUARD,), -7.0, dtype=torch.float64, device="cuda")
            else:
                t[name] = torch.full((n + GUARD,), -7, dtype=torch.int64 if name == "bad" else torch.int32, device="cuda")
        spec = bands_spec(S, n_bins, first, last, weights, m, R, T, seed, dbins.data_ptr())
        rc = L.r3d_envelope_bands(0, B, dx.data_ptr(), C.byref(spec), *[t[name].data_ptr() if name in ask else None for name in NAMES],
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.r3d_last_error().decode()
        torch.cuda.synchronize()
        got = {}
        for name, n in sizes.items():
            if name not in ask:
                assert (t[name] == -7).all(), name                  # (not asked for: not touched)
                got[name] = None
                continue
            assert (t[name][n:] == -7).all(), name
            got[name] = t[name][:n].cpu().numpy()
        outs.append(got)
    assert torch.equal(dx.view(torch.int64), keep.view(torch.int64)) and torch.equal(dbins, keep_bins)   # (by bits: a block may hold NaN)
    for name in NAMES:
        if outs[0][name] is not None:
            same = bits(outs[0][name]) == bits(outs[1][name]) if name in F64 else outs[0][name] == outs[1][name]
            assert same.all(), name
    return outs[0]


def check_against_host(x, windows, first, last, weights, m, R, T, seed, what, **kw):
    got = run_kernel(x, windows, first, last, weights, m, R, T, seed, **kw)
    want = host_envelope_bands(x, windows, first, last, weights, m, R, T, seed)
    for name in F64:                                                # bit for bit: the sign of a zero and every NaN included
        if got[name] is not None:
            off = np.flatnonzero(bits(got[name]) != bits(want[name].reshape(-1)))[:8]
            assert off.size == 0, (what, name, off.tolist(), got[name][off].tolist(), want[name].reshape(-1)[off].tolist())
    if got["defined"] is not None:
        assert (got["defined"].view(np.uint32) == want["defined"].reshape(-1)).all(), (what, "defined")
    if got["bad"] is not None:
        assert int(got["bad"][0]) == want["bad"], what
    return got, want


# ---- the kernels alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", LENGTHS)
def test_envelope_bands_kernel_equals_the_host_build_bit_for_bit(length):
    """Every window length around the kernel's 64-bin tile, starting off the tile boundary, for every B and R; the passes, A (3:
    with a row dominated by one batch and a zero row), the three weight sets and the two tails (0 and the largest 2 T < R allows)
    go round underneath, so that every one of them meets every B and several R at every length."""
    rng = np.random.default_rng(9500 + length)
    n = 0
    for B in BATCHES:
        x = planted_blocks(B, N_BINS, rng)
        for R in REPLICATES:
            for A in (1, 3):
                m, weights, T = SMOOTH[n % 3], WEIGHTS[(n // 3) % 3], (0, (R - 1) // 2)[(n // 2) % 2]
                windows = [[STARTS[(n + i) % 3], STARTS[(n + i) % 3] + length] for i in range(A)]
                n += 1
                got, want = check_against_host(x, windows, FIRST, FIRST + A - 1, weights, m, R, T, 0xB007 + n, (length, B, R, A, m, T))
                D = want["defined"]
                assert (D[:, :2] == R).all() and (want["envelope_lo"] <= want["envelope_hi"]).all()
                if length == 0:
                    assert (D[:, 2:] == 0).all() and (bits(got["shape_lo"].reshape(A, 6)[:, 2:]) == NAN_BITS).all()
                    assert all((bits(got[k]) == 0).all() for k in F64[:3])
                elif A == 3:
                    assert (D[2, 2:] == 0).all() and (D[:2, [TP, CEN, WID]] == R).all()                  # the zero row; the living ones
                    assert all((bits(got[k].reshape(3, N_BINS)[2]) == 0).all() for k in F64[:3])
                    assert np.isfinite(got["shape_lo"].reshape(3, 6)[:2, [E_, P_, TP, CEN, WID]]).all()


def test_device_counts_are_the_host_counts():
    L = _ffi.hip_lib()
    for seed, B, R in ((0, 2, 1), (0x5EED, 3, 257), (0xFFFFFFFF00000001, 64, 65), (77 << 32, 61, 4096)):
        d = torch.full((R * B + GUARD,), 99, dtype=torch.uint8, device="cuda")
        assert L.r3d_bootstrap_counts_device(0, seed, B, R, d.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert (d[R * B:] == 99).all()
        assert (d[:R * B].cpu().numpy().reshape(R, B) == bootstrap_counts(seed, B, R)).all(), (seed, B, R)
    for args in ((2, 1, 4), (2, 65, 4), (2, 4, 0), (2, 4, 4097)):
        assert L.r3d_bootstrap_counts_device(0, *args, d.data_ptr(), None) != 0
        assert L.r3d_last_error().decode().startswith("r3d_bootstrap_counts_device: ")


def test_planted_edge_rows_and_bad_or_clipped_windows():
    """The CPU test's planted rows, in blocks: a tied peak, the peak in the first and in the last bin, a row that never falls to
    half, a zero row, a row that only some replicates see decay (defined < R); then windows that are cut at n_bins, empty,
    reversed or past the blocks, with NaN planted behind them."""
    for B in (2, 3, 8):
        x = rows_as_blocks(planted_batches(B), S=10, first=1)
        for m, R, T in ((0, 37, 5), (1, 64, 9), (4, 37, 18)):
            got, want = check_against_host(x, [[0, 12]] * 8, 1, 8, ONLY_X, m, R, T, 0xB0 + B, ("edges", B, m, R, T))
            D = want["defined"]
            assert (D[[5, 7]] == [R, R, 0, 0, 0, 0]).all()
            if B == 3 and m == 0:
                assert 0 < D[6, TQ] < R and D[3, TQ] == 0
    rng = np.random.default_rng(9600)
    x = planted_blocks(3, N_BINS, rng)
    x[:, FIRST + 2] = np.nan                                                                              # never read through
    windows = [[150, N_BINS], [70, 70], [9, 3]]
    got, want = check_against_host(x, windows, FIRST, FIRST + 2, WEIGHTS[2], 8, 65, 3, 11, "cut, empty, reversed")
    assert int(got["bad"][0]) == 1 and (want["defined"][1:, 2:] == 0).all() and (want["defined"][0] == 65).sum() >= 5
    got, want = check_against_host(x, [[0, N_BINS + 1]], FIRST + 2, FIRST + 2, WEIGHTS[2], 8, 65, 3, 11, "past the blocks")
    assert int(got["bad"][0]) == 1 and all((bits(got[k]) == 0).all() for k in F64[:3])


def test_more_receivers_than_workgroups_of_one_launch():
    """700 receivers of 70 bins, R = 64: a workgroup serves several of them in turn, through the same scratch rows."""
    rng = np.random.default_rng(9650)
    A, n_bins = 700, 70
    x = rng.lognormal(0.0, 1.0, (3, A + 1, n_bins, 5))
    x[:, 1::7, :40] = 0.0
    x[:, 5::50] = 0.0
    windows = [[i % 5, n_bins - i % 3] for i in range(A)]
    got, want = check_against_host(x, windows, 1, A, WEIGHTS[2], 3, 64, 3, 21, "700 receivers")
    assert (want["defined"][:, TP] == 64).sum() == A - len(range(4, A, 50))


def test_outputs_that_are_not_asked_for_are_not_touched():
    rng = np.random.default_rng(9700)
    x = planted_blocks(3, N_BINS, rng)
    windows = [[1, 131], [63, 193], [64, 128]]
    full, _ = check_against_host(x, windows, FIRST, FIRST + 2, WEIGHTS[0], 8, 65, 4, 5, "all")
    for ask in ((), ("shape",), ("envelope_hi",), ("shape_lo", "bad"), ("envelope", "defined"), ("envelope_lo", "shape_hi")):
        got, _ = check_against_host(x, windows, FIRST, FIRST + 2, WEIGHTS[0], 8, 65, 4, 5, ask, ask=ask)
        assert all((bits(got[k]) == bits(full[k])).all() for k in ask if k in F64)


def test_the_point_estimate_is_r3d_envelope_shapes_on_the_same_blocks():
    rng = np.random.default_rng(9800)
    for B, m in ((2, 0), (3, 8), (64, 1)):
        x = planted_blocks(B, N_BINS, rng)
        dx = torch.from_numpy(x).cuda()
        windows = torch.tensor([[1, 131], [63, 200], [64, 128]], dtype=torch.int32, device="cuda")
        for weights in WEIGHTS:
            bands = envelope_bands(dx, windows, FIRST, FIRST + 2, weights, m, n_replicates=5, tail=1, seed=3)
            shp = envelope_shape(dx, windows, FIRST, FIRST + 2, weights, m)
            torch.cuda.synchronize()
            for name in ("envelope", "shape"):
                assert (bits(bands[name].cpu().numpy()) == bits(shp[name].cpu().numpy())).all(), (B, m, name)
            assert (shp["shape"][:2, P_] > 0).all() and int(bands["bad"][0]) == 0


def test_refusals_enqueue_nothing():
    L = _ffi.hip_lib()
    x = torch.full((2, 5, 40, 5), 1.5, dtype=torch.float64, device="cuda")
    bins = torch.tensor([[0, 40]] * 3, dtype=torch.int32, device="cuda")
    out = {n: torch.full((3 * 40,), -7.0, dtype=torch.float64, device="cuda") for n in F64}
    ints = {n: torch.full((24,), -7, dtype=torch.int64, device="cuda") for n in ("defined", "bad")}

    def call(B=2, blocks=x.data_ptr(), spec="spec", **kw):
        s = bands_spec(5, kw.pop("n_bins", 40), kw.pop("first", 1), kw.pop("last", 3), kw.pop("weights", (1, 1, 1, 0, 0)),
                       kw.pop("smooth", 8), kw.pop("R", 9), kw.pop("T", 2), 5, kw.pop("bins", bins.data_ptr()))
        for key, v in kw.items():
            setattr(s, key, v)
        return L.r3d_envelope_bands(0, B, blocks, C.byref(s) if spec else None, *[out[n].data_ptr() for n in F64],
                                    ints["defined"].data_ptr(), ints["bad"].data_ptr(), None)

    # (n_bins = 65600 with 4096 replicates: 2 x 4097 x 65600 + 6 x 4096 doubles for ONE receiver, above the cap of 2^29)
    refused = [dict(blocks=None), dict(spec=None), dict(bins=None), dict(size=4), dict(B=0), dict(B=1), dict(B=65), dict(R=0),
               dict(R=4097), dict(R=9, T=5), dict(R=8, T=4), dict(R=1, T=1), dict(n_bins=0), dict(first=3, last=2), dict(last=5),
               dict(weights=(1, -1, 1, 0, 0)), dict(weights=(1, math.inf, 1, 0, 0)), dict(weights=(math.nan, 1, 1, 0, 0)),
               dict(smooth=65), dict(R=4096, n_bins=65600)]
    for kw in refused:
        assert call(**dict(kw)) != 0, kw
        assert L.r3d_last_error().decode().startswith("r3d_envelope_bands: "), kw
    assert "exceed the cap" in L.r3d_last_error().decode()
    torch.cuda.synchronize()
    assert all((t == -7.0).all() for t in out.values()) and all((t == -7).all() for t in ints.values())
    assert call() == 0 and call(R=9, T=4) == 0 and call(R=1, T=0, smooth=0) == 0              # and these go through
    torch.cuda.synchronize()
    assert (out["shape"][:18].reshape(3, 6)[:, :2] > 0).all() and (out["shape_lo"][:18].reshape(3, 6)[:, :2] > 0).all()


# ---- real blocks, and the run that does it all ---------------------------------------------------------------------------
AXES = (1.0, 1.0, 1.0, 0.0, 0.0)
N, B_RUN, SEED, M_RUN, R_RUN, T_RUN, BANDS_SEED = 50000, 10, 0x5EED, 8, 200, 10, 0xB007


@pytest.fixture(scope="module")
def engine(models):
    e = Engine(models("halfspace", 4), reproducible=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def composed(engine):
    """The kept blocks of one batched run and what r3d_envelope_bands makes of them on the device: computed once, shared, left
    unchanged."""
    m = engine.model
    S = m.n_seismometers
    dist, bins, clipped = m.envshape_plan(dict(first=0, last=S - 1))
    res, ese, cse, be, bc = engine.run_batched(N, B_RUN, seed=SEED, keep_batches=True)
    dbe = torch.from_numpy(be).cuda()
    out = envelope_bands(dbe, torch.from_numpy(bins.view(np.int32)).cuda(), 0, S - 1, AXES, M_RUN, R_RUN, T_RUN, BANDS_SEED)
    torch.cuda.synchronize()
    assert torch.equal(dbe, torch.from_numpy(be).cuda())
    return dict(bins=bins, res=res, ese=ese, cse=cse, be=be, got={k: v.cpu().numpy() for k, v in out.items()})


def test_bands_on_the_blocks_of_a_real_run_equal_the_host_build(composed):
    k = composed
    S = k["be"].shape[1]
    want = host_envelope_bands(k["be"], k["bins"], 0, S - 1, AXES, M_RUN, R_RUN, T_RUN, BANDS_SEED)
    for name in F64:
        assert (bits(k["got"][name]) == bits(want[name])).all(), name
    assert (k["got"]["defined"].view(np.uint32) == want["defined"]).all() and int(k["got"]["bad"][0]) == 0
    lit = want["shape"][:, P_] > 0
    lo, hi, env = want["envelope_lo"], want["envelope_hi"], want["envelope"]
    inside = ((lo <= env) & (env <= hi)).mean()
    print(f"{lit.sum()} of {S} rows lit; the point envelope lies within its own band in {inside:.3f} of the bins; "
          f"replicates with a half time: {want['defined'][lit, TQ].mean():.1f} of {R_RUN}")
    assert lit.any() and (lo >= 0).all() and (lo <= hi).all() and inside > 0.9
    assert (want["shape_lo"][lit][:, [E_, P_, CEN, WID]] <= want["shape_hi"][lit][:, [E_, P_, CEN, WID]]).all()


def test_run_batched_envelope_bands_equals_the_composition(engine, composed):
    """The run against the device-level call on ANOTHER run's kept blocks.  Two runs of the same histories agree to summation order
    and not to the bit; tests/test_envelope_shape_gpu.py derives the relative move r = 3e-11 PS_b / t_b that the parity figure
    allows a bin's weighted energy, and that every value of a smoothed row -- a combination of such bins with non-negative
    weights, which a replicate row is as well -- then moves by at most r of itself.
    HOW THE BINS ARE DECIDED: none has to be left out.  An order statistic is a monotone function of its values: if every one of
    the R values moves by at most r of itself, the k-th smallest of the moved values lies within r of the k-th smallest of the
    unmoved ones, whether or not any two replicates change places.  So lo and hi are held to r at EVERY bin, and so are the lo and
    hi of E and P; those of the centroid to 2 r n_bins and of the width to 3 r n_bins (the shape test's moves, at the largest
    centroid a window has).  `defined` must agree wherever it counts rows that are alive (all but tq); tp and tq are positions that
    jump with the order of two bins and are only counted."""
    k = composed
    S, n_bins = k["be"].shape[1:3]
    res, ese, cse, bands = engine.run_batched_envelope_bands(N, B_RUN, k["bins"], 0, S - 1, AXES, M_RUN, R_RUN, T_RUN, BANDS_SEED,
                                                             seed=SEED)
    assert (res.counts == k["res"].counts).all() and (res.scalars() == k["res"].scalars()).all()
    from tests.test_gpu_parity import energies_agree
    ps = k["be"].sum(axis=0)[..., 3:].sum(-1)
    assert energies_agree(k["res"].energy, res.energy) and np.allclose(cse, k["cse"], rtol=1e-12, atol=0)
    assert np.allclose(ese, k["ese"], rtol=1e-6, atol=1e-11 * ps.max())
    t = k["be"].sum(axis=0)[..., :3].sum(-1)
    with np.errstate(all="ignore"):
        r = np.where(t > 0, 3e-11 * ps / t, 0.0).max(axis=1)
    print(f"largest relative move of a bin's weighted energy that the parity figure allows: {r.max():.3g}")
    assert r.max() < 1e-9
    want = k["got"]
    for name in ("envelope", "envelope_lo", "envelope_hi"):
        assert (np.abs(bands[name] - want[name]) <= r[:, None] * want[name]).all(), name
    D, wD = bands["defined"], want["defined"].view(np.uint32)
    assert (D[:, [E_, P_, TP, CEN, WID]] == wD[:, [E_, P_, TP, CEN, WID]]).all()
    lit = want["shape"][:, P_] > 0
    assert lit.any() and ((bands["shape"][:, P_] > 0) == lit).all()
    for name in ("shape", "shape_lo", "shape_hi"):
        g, w = bands[name], want[name]
        assert (np.abs(g[:, E_] - w[:, E_]) <= r * w[:, E_]).all() and (np.abs(g[:, P_] - w[:, P_]) <= r * w[:, P_]).all(), name
        assert (np.abs(g[lit, CEN] - w[lit, CEN]) <= 2 * r[lit] * n_bins + 1e-300).all(), name
        assert (np.abs(g[lit, WID] - w[lit, WID]) <= 3 * r[lit] * n_bins + 1e-300).all(), name
    off = sum(int((bits(bands[name]) != bits(want[name])).sum()) for name in F64)
    moved = int((bits(bands["shape_lo"][:, [TP, TQ]]) != bits(want["shape_lo"][:, [TP, TQ]])).sum() +
                (bits(bands["shape_hi"][:, [TP, TQ]]) != bits(want["shape_hi"][:, [TP, TQ]])).sum())
    print(f"entries whose bits differ between the run and the call on a second run's blocks: {off} of {sum(want[n].size for n in F64)}; "
          f"lo / hi of tp and tq among them: {moved}; defined(tq) differs at {int((D[:, TQ] != wD[:, TQ]).sum())} receivers")


def test_a_refused_run_touches_nothing(engine):
    m = engine.model
    L = engine._lib
    S, n_bins = m.n_seismometers, m.n_bins
    A = S - 2
    _, bins, _ = m.envshape_plan(dict(first=1, last=S - 2))

    def fresh():
        res = m.new_result()
        res.energy[:], res.counts[:] = 3.5, 7
        bufs = dict(res=res, ese=np.full(res.energy.shape, -1.0), cse=np.full(res.counts.shape, -1.0))
        bufs.update({key: np.full((A, n_bins), -2.0) for key in F64[:3]})
        bufs.update({key: np.full((A, 6), -2.0) for key in F64[3:]})
        bufs["defined"] = np.full((A, 6), 9, dtype=np.uint32)
        return bufs

    def call(n, batches, bufs, bins=bins, size=None, result=True, R=50, T=2, **spec_kw):
        b = np.ascontiguousarray(bins, dtype=np.uint32)
        spec = bands_spec(S, n_bins, 1, S - 2, AXES, M_RUN, R, T, BANDS_SEED, b.ctypes.data)
        for key, v in spec_kw.items():
            setattr(spec, key, v)
        out = _ffi.BandsResult(size=C.sizeof(_ffi.BandsResult) if size is None else size,
                               **{key: v.ctypes.data for key, v in bufs.items() if key not in ("res", "ese", "cse")})
        c = bufs["res"]._as_c()
        rc = L.r3d_run_batched_envelope_bands(engine._e, n, 0, SEED, batches, C.byref(c), bufs["ese"].ctypes.data_as(_ffi._dp),
                                              bufs["cse"].ctypes.data_as(_ffi._dp), C.byref(spec), C.byref(out) if result else None)
        bufs["res"]._from_c(c)
        return rc

    def refused(n, batches, match, **kw):
        bufs = fresh()
        assert call(n, batches, bufs, **kw) != 0 and match in L.r3d_last_error().decode(), L.r3d_last_error().decode()
        assert L.r3d_last_error().decode().startswith("r3d_run_batched_envelope_bands: ")
        r = bufs["res"]
        assert (r.energy == 3.5).all() and (r.counts == 7).all() and not r.scalars().any()
        assert (bufs["ese"] == -1.0).all() and (bufs["cse"] == -1.0).all()
        assert all((bufs[key] == -2.0).all() for key in F64) and (bufs["defined"] == 9).all()

    refused(1000, 1, "at least 2 batches")
    refused(1000, 65, "at most 64 batches")
    refused(3, 4, "fewer histories")
    refused(1000, 4, "not the model's", n_bins=n_bins - 1)
    refused(1000, 4, "negative or not finite", weight=(C.c_double * 5)(0, 0, -1.0, 0, 0))
    refused(1000, 4, "R3D_ENVELOPE_MAX_SMOOTH", smooth=65)
    refused(1000, 4, "R3D_BANDS_MAX_REPLICATES", R=0)
    refused(1000, 4, "R3D_BANDS_MAX_REPLICATES", R=4097, T=0)
    refused(1000, 4, "2 tail < n_replicates", R=50, T=25)
    bad = bins.copy()
    bad[3] = [9, 3]
    refused(1000, 4, "receiver 3 of the array is not begin <= end <= n_bins", bins=bad)
    bad[3] = [0, n_bins + 1]
    refused(1000, 4, "receiver 3 of the array", bins=bad)
    refused(1000, 4, "null bands result", result=False)
    refused(1000, 4, "r3d_bands_result.size", size=8)
    with pytest.raises(RuntimeError, match="at least 2 batches"):
        engine.run_batched_envelope_bands(1000, 1, bins, 1, S - 2, AXES)
    # with all of that gone the same call goes through, and everything is WRITTEN
    bufs = fresh()
    assert call(4000, 4, bufs) == 0, L.r3d_last_error().decode()
    assert (bufs["res"].counts - 7 == engine.run(4000, seed=SEED).counts).all()
    assert all((bufs[key] >= 0).all() for key in F64[:3]) and (bufs["shape"][:, :2] >= 0).all() and (bufs["defined"] <= 50).all()


# ---- ./main --envelope-bands ---------------------------------------------------------------------------------------------------
def test_cli_envelope_bands_end_to_end(tmp_path):
    import subprocess

    from cli_support import main_exe
    from octave_text import read_octave
    from radiative3d_amd import Model
    from tests.configs import halfspace
    args = halfspace(4) + ["--num-phonons=2M", "--seed=77", "--error-batches=8"]
    extra = ["--envelope-bands=200,0.9,3.6,0,-2,60,4", "--bands-array=48,95", "--bands-seed=11"]
    plain, env = tmp_path / "plain", tmp_path / "env"
    plain.mkdir(), env.mkdir()
    for out, more in ((plain, []), (env, extra)):
        r = subprocess.run([main_exe()] + args + [f"--output-dir={out}"] + more, cwd=out, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert not (plain / "envbands.octv").exists()
    # the seis and err files are what they are without the bands' options, byte for byte
    names = sorted(p.name for p in plain.glob("seis_*.octv"))
    assert len(names) == 288 and names == sorted(p.name for p in env.glob("seis_*.octv"))
    for name in names:
        assert (plain / name).read_bytes() == (env / name).read_bytes(), name
    got = read_octave(env / "envbands.octv")
    n_bins, dt = 400, 0.5
    assert (got["BandsSeismometers"][:, 0] == np.arange(48, 96)).all() and got["BandsBatches"] == 8 and got["BandsNumBins"] == n_bins
    assert got["BandsReplicates"] == 200 and got["BandsSeed"] == 11 and got["BandsSmooth"] == 4
    assert got["BandsAxes"].tolist() == [[1, 1, 1]] and got["BandsWindow"].tolist() == [[-2, 60]]
    # the same run through the API
    model = Model(args + extra)
    rq = model.envbands_request
    T = rq["tail"]
    assert T == math.floor((0.5 * (1.0 - 0.9)) * 200.0) and got["BandsTail"] == T and got["BandsLevel"] == 1.0 - 2.0 * T / 200.0
    dist, bins, clipped = model.envbands_plan()
    assert (got["BandsDistances"][:, 0] == dist).all() and (got["BandsBins"] == bins).all() and (got["BandsClipped"][:, 0] == clipped).all()
    e = Engine(model)
    _, _, _, bands = e.run_batched_envelope_bands(model.num_phonons, 8, bins, 48, 95, AXES, 4, 200, T, 11, seed=77)
    e.close()
    lit = bands["shape"][:, P_] > 0
    assert lit.sum() >= 10
    close = lambda a, b: np.allclose(a, b, rtol=1e-8, atol=0, equal_nan=True)                           # noqa: E731
    for tail_name, key in (("", "shape"), ("_lo", "shape_lo"), ("_hi", "shape_hi")):
        six = bands[key]
        assert close(got["BandsEnergy" + tail_name][:, 0], six[:, E_] * dt) and close(got["BandsPeak" + tail_name][:, 0], six[:, P_])
        assert close(got["BandsCentroid" + tail_name][:, 0], (six[:, CEN] + 0.5) * dt), tail_name
        assert close(got["BandsWidth" + tail_name][:, 0], six[:, WID] * dt), tail_name
    for q, name in ((E_, "BandsEnergy"), (P_, "BandsPeak"), (TP, "BandsPeakTime"), (CEN, "BandsCentroid"), (WID, "BandsWidth")):
        assert (got[name + "_defined"][:, 0] == bands["defined"][:, q]).all(), name
    for name, key in (("BandsEnvelope", "envelope"), ("BandsEnvelope_lo", "envelope_lo"), ("BandsEnvelope_hi", "envelope_hi")):
        assert close(got[name], bands[key]) and (got[name][:, :bins[:, 0].min()] == 0).all(), name
    assert (got["BandsEnvelope_lo"] >= 0).all() and (got["BandsEnvelope_lo"] <= got["BandsEnvelope_hi"]).all()
    # positions: two runs differ by summation order, which moves a position only where two bins, or two replicates, are level
    agree = np.isclose(got["BandsPeakTime_lo"][:, 0], (bands["shape_lo"][:, TP] + 0.5) * dt, rtol=0, atol=1e-6, equal_nan=True)
    assert agree.mean() >= 0.9
