"""The envelope shape per receiver with jackknife errors on the GPU: the kernel (r3d_envelope_shape) against the host build of
the lines it runs, bit for bit; against its siblings where they compute the same thing; on the kept blocks of a real batched
run; the run that does all of it where the blocks lie (r3d_run_batched_envelope_shape); and ./main --envelope-shape end to
end."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest
import torch

from array_image_cases import WEIGHTS
from cli_support import main_exe
from envelope_cases import (BATCHES, CEN, E_, FIRST, LENGTHS, N_BINS, NAN_BITS, NO_BIN, ONLY_X, P_, S_ALL, SMOOTH, STARTS, TP, TQ,
                            WID, bits, host_envelope_shape, planted_blocks, rows_as_blocks)
from octave_text import read_octave
from radiative3d_amd import Engine, Model, _ffi, array_image, envelope_shape, window_sums
from radiative3d_amd.model import envelope_spec
from tests.configs import halfspace

pytestmark = pytest.mark.gpu

GUARD = 64
F64 = ("shape", "shape_se", "envelope", "envelope_se")
U32 = ("peak_bin", "half_bin", "lit")


def run_kernel(x, windows, first, last, weights, m, ask=F64 + U32 + ("bad",)):
    """r3d_envelope_shape into guarded outputs, twice: the outputs as numpy, after the checks that belong to every launch --
    the second run has the first one's bits, the blocks and the bins are unchanged, the guards behind every output stand, an
    output that was not asked for (not in `ask`, or an se with B < 2) is untouched."""
    L = _ffi.hip_lib()
    B, S, n_bins = x.shape[:3]
    A = last - first + 1
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dbins = torch.from_numpy(np.ascontiguousarray(windows, dtype=np.uint32).view(np.int32).reshape(A, 2)).cuda()
    keep, keep_bins = dx.clone(), dbins.clone()
    sizes = dict(shape=A * 6, shape_se=A * 6, envelope=A * n_bins, envelope_se=A * n_bins, peak_bin=A, half_bin=A, lit=A, bad=1)
    asked = {name: name in ask and not (name.endswith("_se") and B < 2) for name in sizes}
    outs = []
    for _ in range(2):
        t = {}
        for name, n in sizes.items():
            if name in F64:
                t[name] = torch.full((n + GUARD,), -7.0, dtype=torch.float64, device="cuda")
            else:
                t[name] = torch.full((n + GUARD,), -7, dtype=torch.int64 if name == "bad" else torch.int32, device="cuda")
        spec = envelope_spec(S, n_bins, first, last, weights, m, dbins.data_ptr())
        rc = L.r3d_envelope_shape(0, B, dx.data_ptr(), C.byref(spec), *[t[name].data_ptr() if asked[name] else None for name in sizes],
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
    assert torch.equal(dx.view(torch.int64), keep.view(torch.int64)) and torch.equal(dbins, keep_bins)   # (by bits: a block may hold NaN)
    for name in sizes:
        if outs[0][name] is not None:
            same = bits(outs[0][name]) == bits(outs[1][name]) if name in F64 else outs[0][name] == outs[1][name]
            assert same.all(), name
    return outs[0]


def check_against_host(x, windows, first, last, weights, m, what, **kw):
    got = run_kernel(x, windows, first, last, weights, m, **kw)
    want = host_envelope_shape(x, windows, first, last, weights, m)
    for name in F64:                                                # bit for bit: the sign of a zero and every NaN included
        if got[name] is not None:
            off = np.flatnonzero(bits(got[name]) != bits(want[name].reshape(-1)))[:8]
            assert off.size == 0, (what, name, off.tolist(), got[name][off].tolist(), want[name].reshape(-1)[off].tolist())
    for name in U32:
        if got[name] is not None:
            assert (got[name].view(np.uint32) == want[name]).all(), (what, name)
    if got["bad"] is not None:
        assert int(got["bad"][0]) == want["bad"], what
    return got, want


# ---- the kernel alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", LENGTHS + (136,))                # 136: from bin 64 to the last of the 200
def test_envelope_shape_kernel_equals_the_host_build_bit_for_bit(length):
    """Every window length around the 64 strands and the kernel's 64-bin tile (nothing else of a row stays on chip, so 65, 130
    and 136 are all lengths above it), starting off the tile boundary, for every B, m, A and the three weight sets."""
    rng = np.random.default_rng(9000 + length)
    n = 0
    for B in BATCHES:
        x = planted_blocks(B, N_BINS, rng)
        for A in (1, 3):
            for m in SMOOTH:
                weights = WEIGHTS[n % 3]
                windows = [[STARTS[(n + i) % 3], STARTS[(n + i) % 3] + length] for i in range(A)]
                n += 1
                got, want = check_against_host(x, windows, FIRST, FIRST + A - 1, weights, m, (length, B, A, m))
                nan = bits(got["shape"]) == NAN_BITS
                if length == 0:
                    assert want["lit"].tolist() == [0] * A and nan.reshape(A, 6)[:, 2:].all()
                elif A == 3:
                    assert want["lit"].tolist() == [1, 1, 0]
                    assert (bits(got["envelope"].reshape(3, N_BINS)[2]) == 0).all()                     # the zero row: +0.0
                    assert nan.reshape(3, 6)[2, 2:].all() and (bits(got["shape"].reshape(3, 6)[2, :2]) == 0).all()
                    assert np.isfinite(got["shape"].reshape(3, 6)[:2, [E_, P_, TP, CEN, WID]]).all()


def test_planted_edge_rows_and_bad_or_clipped_windows():
    """The CPU test's edge rows, in blocks: a tied peak, the peak in the first and in the last bin, a row that never falls to
    half, u[kq] == h exactly, a zero row -- as equal batches (every se +0.0 or NaN) and with one batch scaled; then windows
    that are cut at n_bins, empty, reversed or past the blocks."""
    rows = np.zeros((8, 12))
    rows[0, 3:7] = [1, 7, 7, 1]
    rows[1, :4] = [9, 5, 1, 0]
    rows[2, 8:] = [0, 1, 5, 9]
    rows[3, 2:6] = [4, 5, 4, 3]
    rows[3, :2], rows[3, 6:] = 3, 3
    rows[4, 4:7] = [0, 8, 0]
    rows[6] = 2.0
    windows = [[0, 12]] * 8
    for B in (1, 2, 3):
        for scale in (1.0, 1e12):
            batches = np.repeat(rows[None], B, axis=0)
            batches[B // 2] *= scale
            x = rows_as_blocks(batches, S=9, first=1)
            for m in (0, 1):
                got, want = check_against_host(x, windows, 1, 8, ONLY_X, m, ("edges", B, scale, m))
                pb, hb = got["peak_bin"].view(np.uint32), got["half_bin"].view(np.uint32)
                if m == 0:
                    assert pb[:5].tolist() == [4, 0, 11, 3, 5] and hb[:5].tolist() == [6, 2, NO_BIN, NO_BIN, 6]
                else:
                    assert hb[4] == 6 and got["shape"].reshape(8, 6)[4, TQ] == 6.0                       # u = [2, 4, 2] from bin 4
                assert got["lit"].tolist() == [1, 1, 1, 1, 1, 0, 1, 0] and pb[5] == NO_BIN
                if B >= 2 and scale == 1.0 and B <= 4:
                    se = got["shape_se"].reshape(8, 6)
                    assert ((bits(se) == 0) | (bits(se) == NAN_BITS)).all()
    rng = np.random.default_rng(9100)
    x = planted_blocks(3, N_BINS, rng)
    x[:, FIRST + 2] = np.nan                                                                              # never read through
    windows = [[150, N_BINS], [70, 70], [9, 3]]
    got, _ = check_against_host(x, windows, FIRST, FIRST + 2, WEIGHTS[2], 8, "cut, empty, reversed")
    assert int(got["bad"][0]) == 1 and got["lit"].tolist() == [1, 0, 0]
    got, _ = check_against_host(x, [[0, N_BINS + 1]], FIRST + 2, FIRST + 2, WEIGHTS[2], 8, "past the blocks")
    assert int(got["bad"][0]) == 1 and got["lit"].tolist() == [0]


def test_more_receivers_than_workgroups_of_one_launch():
    """700 receivers: a workgroup serves several of them in turn, through the same scratch rows."""
    rng = np.random.default_rng(9150)
    A, n_bins = 700, 70
    x = rng.lognormal(0.0, 1.0, (3, A + 1, n_bins, 5))
    x[:, 1::7, :40] = 0.0
    x[:, 5::50] = 0.0
    windows = [[i % 5, n_bins - i % 3] for i in range(A)]
    got, want = check_against_host(x, windows, 1, A, WEIGHTS[2], 3, "700 receivers")
    assert want["lit"].sum() == A - len(range(4, A, 50)) and np.isfinite(want["shape_se"][want["lit"] == 1][:, :2]).all()


def test_outputs_that_are_not_asked_for_are_not_touched():
    rng = np.random.default_rng(9200)
    x = planted_blocks(3, N_BINS, rng)
    windows = [[1, 131], [63, 193], [64, 128]]
    full, _ = check_against_host(x, windows, FIRST, FIRST + 2, WEIGHTS[0], 8, "all")
    for ask in (("shape",), ("shape", "envelope_se"), ("shape", "shape_se", "lit"), ("shape", "envelope", "half_bin", "bad")):
        got, _ = check_against_host(x, windows, FIRST, FIRST + 2, WEIGHTS[0], 8, ask, ask=ask)
        assert (bits(got["shape"]) == bits(full["shape"])).all()


def test_receivers_whose_offset_passes_2_to_31_doubles():
    """[2][S][130][5] with S * 650 > 2^31: the array is the last three receivers, whose bins lie past a 32-bit offset in both
    blocks (and the second block's start does too)."""
    rng = np.random.default_rng(9300)
    n_bins = 130
    S = (1 << 31) // (n_bins * 5) + 7
    tail = planted_blocks(2, n_bins, rng)[:, FIRST:FIRST + 3]
    tail[:, 2] = tail[:, 0][:, ::-1]                                                                     # (no zero row here)
    x = torch.zeros((2, S, n_bins, 5), dtype=torch.float64, device="cuda")
    x[:, S - 3:] = torch.from_numpy(tail).cuda()
    windows = np.array([[1, 130], [0, 65], [64, 129]], dtype=np.int32)
    out = envelope_shape(x, torch.from_numpy(windows).cuda(), S - 3, S - 1, WEIGHTS[2], 8)
    torch.cuda.synchronize()
    want = host_envelope_shape(tail, windows, 0, 2, WEIGHTS[2], 8)
    for name in F64:
        assert (bits(out[name].cpu().numpy()) == bits(want[name])).all(), name
    for name in U32:
        assert (out[name].cpu().numpy().view(np.uint32) == want[name]).all(), name
    assert (want["shape"][:, P_] > 0).all() and int(out["bad"][0]) == 0


def test_refusals_enqueue_nothing():
    L = _ffi.hip_lib()
    x = torch.full((2, 5, 40, 5), 1.5, dtype=torch.float64, device="cuda")
    bins = torch.tensor([[0, 40]] * 3, dtype=torch.int32, device="cuda")
    out = {n: torch.full((3 * 40,), -7.0, dtype=torch.float64, device="cuda") for n in ("shape", "se", "env", "env_se")}
    ints = {n: torch.full((8,), -7, dtype=torch.int64, device="cuda") for n in ("peak", "half", "lit", "bad")}

    def call(B=2, blocks=x.data_ptr(), shape=out["shape"].data_ptr(), se=out["se"].data_ptr(), env_se=out["env_se"].data_ptr(),
             spec="spec", **kw):
        s = envelope_spec(5, kw.pop("n_bins", 40), kw.pop("first", 1), kw.pop("last", 3), kw.pop("weights", (1, 1, 1, 0, 0)),
                          kw.pop("smooth", 8), kw.pop("bins", bins.data_ptr()))
        for key, v in kw.items():
            setattr(s, key, v)
        return L.r3d_envelope_shape(0, B, blocks, C.byref(s) if spec else None, shape, se, out["env"].data_ptr(), env_se,
                                    ints["peak"].data_ptr(), ints["half"].data_ptr(), ints["lit"].data_ptr(), ints["bad"].data_ptr(),
                                    None)

    refused = [dict(blocks=None), dict(spec=None), dict(shape=None), dict(bins=None), dict(size=4), dict(B=0), dict(B=65),
               dict(n_bins=0), dict(first=3, last=2), dict(last=5), dict(weights=(1, -1, 1, 0, 0)), dict(weights=(1, math.inf, 1, 0, 0)),
               dict(weights=(math.nan, 1, 1, 0, 0)), dict(smooth=65), dict(B=1), dict(B=1, se=None)]
    for kw in refused:
        assert call(**dict(kw)) != 0, kw
        assert L.r3d_last_error().decode().startswith("r3d_envelope_shape: "), kw
    torch.cuda.synchronize()
    assert all((t == -7.0).all() for t in out.values()) and all((t == -7).all() for t in ints.values())
    assert call() == 0 and call(B=1, se=None, env_se=None) == 0 and call(smooth=0) == 0        # and these go through
    torch.cuda.synchronize()
    assert (out["shape"][:18].reshape(3, 6)[:, :2] > 0).all()


# ---- consistency with the siblings ----------------------------------------------------------------------------------------
def test_energy_and_peak_are_the_siblings_on_one_plain_block():
    """B = 1, no pass, the full window: E is r3d_window_sums' full-window sum of the block, P and the peak's bin are
    r3d_array_image's peak and peak_bin -- bit for bit."""
    rng = np.random.default_rng(9400)
    for n_bins in (65, 130, 400):
        x = planted_blocks(1, n_bins, rng)
        x[0, FIRST + 2] = x[0, FIRST][::-1]
        dx = torch.from_numpy(x).cuda()
        full = torch.tensor([[[0, n_bins]]] * S_ALL, dtype=torch.int32, device="cuda")
        for weights in WEIGHTS:
            out = envelope_shape(dx, full[FIRST:FIRST + 3, 0].contiguous(), FIRST, FIRST + 2, weights, 0)
            y, _, _ = window_sums(dx, full, weights)
            img = array_image(dx, FIRST, FIRST + 2, weights)
            torch.cuda.synchronize()
            shape = out["shape"].cpu().numpy()
            assert (bits(shape[:, E_]) == bits(y[0, FIRST:FIRST + 3, 0].cpu().numpy())).all()
            assert (bits(shape[:, P_]) == bits(img["peak"].cpu().numpy())).all()
            assert (out["peak_bin"].cpu().numpy() == img["peak_bin"].cpu().numpy()).all() and (shape[:, P_] > 0).all()


# ---- real blocks, and the run that does it all ---------------------------------------------------------------------------
AXES = (1.0, 1.0, 1.0, 0.0, 0.0)
N, B_RUN, SEED, M_RUN = 50000, 10, 0x5EED, 8


@pytest.fixture(scope="module")
def engine(models):
    e = Engine(models("halfspace", 4), reproducible=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def composed(engine):
    """The kept blocks of one batched run and what r3d_envelope_shape makes of them on the device: computed once, shared, left
    unchanged."""
    m = engine.model
    S = m.n_seismometers
    dist, bins, clipped = m.envshape_plan(dict(first=0, last=S - 1))
    res, ese, cse, be, bc = engine.run_batched(N, B_RUN, seed=SEED, keep_batches=True)
    dbe = torch.from_numpy(be).cuda()
    out = envelope_shape(dbe, torch.from_numpy(bins.view(np.int32)).cuda(), 0, S - 1, AXES, M_RUN)
    torch.cuda.synchronize()
    assert torch.equal(dbe, torch.from_numpy(be).cuda())
    return dict(bins=bins, res=res, ese=ese, cse=cse, be=be, got={k: v.cpu().numpy() for k, v in out.items()})


def test_shape_on_the_blocks_of_a_real_run_equals_the_host_build(composed):
    k = composed
    S = k["be"].shape[1]
    want = host_envelope_shape(k["be"], k["bins"], 0, S - 1, AXES, M_RUN)
    for name in F64:
        assert (bits(k["got"][name]) == bits(want[name])).all(), name
    for name in U32:
        assert (k["got"][name].view(np.uint32) == want[name]).all(), name
    lit = want["lit"].astype(bool)
    decayed = lit & (want["half_bin"] != NO_BIN)
    print(f"{lit.sum()} of {S} rows lit, {decayed.sum()} of them fall to half their peak; finite se: "
          f"{np.isfinite(want['shape_se']).all(axis=1).sum()}")
    assert lit.any() and decayed.any() and int(k["got"]["bad"][0]) == 0
    assert np.isfinite(want["shape"][lit][:, [E_, P_, TP, CEN, WID]]).all() and (want["shape"][~lit, 0] == 0).all()


def test_run_batched_envelope_shape_equals_the_composition(engine, composed):
    """The run against the device-level call on ANOTHER run's kept blocks, as tests/test_array_image_gpu.py holds its run to its
    kernel.  Two runs of the same histories agree to summation order and not to the bit, on the reproducible build as on the
    other (a few entries in a million of the kept blocks differ in their last bit: the bins are summed by atomic adds);
    tests/test_gpu_parity.energies_agree's figure is 1e-11 of a bin's P + S energy in each component.  With the weights (1, 1, 1, 0, 0) a bin's weighted energy moves by r = 3e-11 PS_b /
    t_b of itself at most, and so does every value of a smoothed row, a convex combination of such bins: E and P move by r,
    the centroid by 2 r of itself, the width by 2 r c + r width (the header's ROUNDINGS with r in place of eps); tp and tq by
    the header's conditional bounds with e = r P, where they hold."""
    k = composed
    m = engine.model
    S, n_bins = k["be"].shape[1:3]
    res, ese, cse, shp = engine.run_batched_envelope_shape(N, B_RUN, k["bins"], 0, S - 1, AXES, M_RUN, seed=SEED)
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
    six, wsix = shp["shape"], want["shape"]
    lit = want["lit"].astype(bool)
    assert (shp["lit"] == want["lit"].view(np.uint32)).all()
    assert (np.abs(six[:, E_] - wsix[:, E_]) <= r * wsix[:, E_]).all() and (np.abs(six[:, P_] - wsix[:, P_]) <= r * wsix[:, P_]).all()
    assert (np.abs(shp["envelope"] - want["envelope"]) <= r[:, None] * want["envelope"]).all()
    c, w = wsix[lit, CEN], wsix[lit, WID]
    assert (np.abs(six[lit, CEN] - c) <= 2 * r[lit] * c + 1e-300).all()
    assert (np.abs(six[lit, WID] - w) <= 2 * r[lit] * c + r[lit] * w + 1e-300).all()
    # the positions, where the device-level rows decide them by more than the figure
    held = 0
    for i in np.flatnonzero(lit):
        b0, b1 = (int(v) for v in k["bins"][i])
        u = want["envelope"][i, b0:b1]
        kp = int(want["peak_bin"][i]) - b0
        e = r[i] * wsix[i, P_]
        if len(u) > 1 and wsix[i, P_] - np.delete(u, kp).max() <= 2 * e:
            continue
        assert shp["peak_bin"][i] == want["peak_bin"].view(np.uint32)[i]
        if 0 < kp < len(u) - 1:
            den = abs((u[kp - 1] - u[kp]) + (u[kp + 1] - u[kp]))
            if den > 8 * e:
                assert abs(six[i, TP] - wsix[i, TP]) <= 4 * e / (den - 4 * e), i
                held += 1
        hb = want["half_bin"].view(np.uint32)[i]
        if hb != NO_BIN and np.abs(u[kp + 1:hb - b0 + 1] - 0.5 * wsix[i, P_]).min() > 2 * e:
            D = u[hb - b0 - 1] - u[hb - b0]
            assert shp["half_bin"][i] == hb
            if D > 8 * e:
                assert abs(six[i, TQ] - wsix[i, TQ]) <= 4 * e / (D - 4 * e), i
    assert held >= 1
    off = int((bits(six) != bits(wsix)).sum() + (bits(shp["shape_se"]) != bits(want["shape_se"])).sum())
    print(f"entries of shape and shape_se whose bits differ between the run and the call on a second run's blocks: {off} of {2 * six.size}")
    # the errors: a jackknife of B values that each move by `move` moves by sqrt(B) times the largest such move
    fin = np.isfinite(want["shape_se"]).all(axis=1) & lit
    assert (np.isfinite(shp["shape_se"]).all(axis=1) == np.isfinite(want["shape_se"]).all(axis=1)).all() and fin.any()
    f = B_RUN / (B_RUN - 1.0)
    for q, move in ((E_, r * wsix[:, E_] * f), (P_, r * wsix[:, P_] * f * 2), (CEN, 2 * r * n_bins), (WID, 3 * r * n_bins)):
        assert (np.abs(shp["shape_se"][fin, q] - want["shape_se"][fin, q]) <= math.sqrt(B_RUN) * 4 * move[fin] + 1e-300).all(), q


def test_a_refused_run_touches_nothing(engine):
    m = engine.model
    L = engine._lib
    S, n_bins = m.n_seismometers, m.n_bins
    A = S - 2
    _, bins, _ = m.envshape_plan(dict(first=1, last=S - 2))

    def fresh():
        res = m.new_result()
        res.energy[:], res.counts[:] = 3.5, 7
        return dict(res=res, ese=np.full(res.energy.shape, -1.0), cse=np.full(res.counts.shape, -1.0), shape=np.full((A, 6), -2.0),
                    shape_se=np.full((A, 6), -2.0), envelope=np.full((A, n_bins), -2.0), envelope_se=np.full((A, n_bins), -2.0),
                    peak_bin=np.full(A, 9, dtype=np.uint32), half_bin=np.full(A, 9, dtype=np.uint32), lit=np.full(A, 9, dtype=np.uint32))

    def call(n, batches, bufs, bins=bins, drop=(), size=None, **spec_kw):
        b = np.ascontiguousarray(bins, dtype=np.uint32)
        spec = envelope_spec(S, n_bins, 1, S - 2, AXES, M_RUN, b.ctypes.data)
        for key, v in spec_kw.items():
            setattr(spec, key, v)
        out = _ffi.EnvelopeResult(size=C.sizeof(_ffi.EnvelopeResult) if size is None else size,
                                  **{key: v.ctypes.data for key, v in bufs.items() if key not in ("res", "ese", "cse") + drop})
        c = bufs["res"]._as_c()
        rc = L.r3d_run_batched_envelope_shape(engine._e, n, 0, SEED, batches, C.byref(c), bufs["ese"].ctypes.data_as(_ffi._dp),
                                              bufs["cse"].ctypes.data_as(_ffi._dp), C.byref(spec), C.byref(out))
        bufs["res"]._from_c(c)
        return rc

    def refused(n, batches, match, **kw):
        bufs = fresh()
        assert call(n, batches, bufs, **kw) != 0 and match in L.r3d_last_error().decode(), L.r3d_last_error().decode()
        r = bufs["res"]
        assert (r.energy == 3.5).all() and (r.counts == 7).all() and not r.scalars().any()
        assert (bufs["ese"] == -1.0).all() and (bufs["cse"] == -1.0).all()
        assert all((bufs[key] == -2.0).all() for key in ("shape", "shape_se", "envelope", "envelope_se"))
        assert all((bufs[key] == 9).all() for key in ("peak_bin", "half_bin", "lit"))

    refused(1000, 1, "at least 2 batches")
    refused(1000, 65, "at most 64 batches")
    refused(3, 4, "fewer histories")
    refused(1000, 4, "not the model's", n_bins=n_bins - 1)
    refused(1000, 4, "negative or not finite", weight=(C.c_double * 5)(0, 0, -1.0, 0, 0))
    refused(1000, 4, "R3D_ENVELOPE_MAX_SMOOTH", smooth=65)
    bad = bins.copy()
    bad[3] = [9, 3]
    refused(1000, 4, "receiver 3 of the array is not begin <= end <= n_bins", bins=bad)
    bad[3] = [0, n_bins + 1]
    refused(1000, 4, "receiver 3 of the array", bins=bad)
    refused(1000, 4, "null shape", drop=("shape_se",))
    refused(1000, 4, "r3d_envelope_result.size", size=8)
    with pytest.raises(RuntimeError, match="at least 2 batches"):
        engine.run_batched_envelope_shape(1000, 1, bins, 1, S - 2, AXES)
    # with all of that gone the same call goes through, and everything is WRITTEN
    bufs = fresh()
    assert call(4000, 4, bufs) == 0, L.r3d_last_error().decode()
    assert (bufs["res"].counts - 7 == engine.run(4000, seed=SEED).counts).all()
    assert (bufs["shape"][:, :2] >= 0).all() and (bufs["envelope"] >= 0).all() and (bufs["lit"] <= 1).all() and bufs["lit"].any()


# ---- ./main --envelope-shape ---------------------------------------------------------------------------------------------------
def test_cli_envelope_shape_end_to_end(tmp_path):
    args = halfspace(4) + ["--num-phonons=2M", "--seed=77", "--error-batches=8"]
    extra = ["--envelope-shape=3.6,0,-2,60,4", "--envelope-array=48,95"]
    plain, env = tmp_path / "plain", tmp_path / "env"
    plain.mkdir(), env.mkdir()
    for out, more in ((plain, []), (env, extra)):
        r = subprocess.run([main_exe()] + args + [f"--output-dir={out}"] + more, cwd=out, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert not (plain / "envshape.octv").exists()
    # the seis and err files are what they are without the shape's options, byte for byte
    names = sorted(p.name for p in plain.glob("seis_*.octv"))
    assert len(names) == 288 and names == sorted(p.name for p in env.glob("seis_*.octv"))
    for name in names:
        assert (plain / name).read_bytes() == (env / name).read_bytes(), name
    got = read_octave(env / "envshape.octv")
    A, n_bins, dt = 48, 400, 0.5
    assert (got["EnvSeismometers"][:, 0] == np.arange(48, 96)).all() and got["EnvBatches"] == 8 and got["EnvNumBins"] == n_bins
    assert got["EnvSmooth"] == 4 and got["EnvAxes"].tolist() == [[1, 1, 1]] and got["EnvWindow"].tolist() == [[-2, 60]]
    # the same run through the API
    model = Model(args + extra)
    dist, bins, clipped = model.envshape_plan()
    assert (got["EnvDistances"][:, 0] == dist).all() and (got["EnvBins"] == bins).all() and (got["EnvClipped"][:, 0] == clipped).all()
    e = Engine(model)
    _, _, _, shp = e.run_batched_envelope_shape(model.num_phonons, 8, bins, 48, 95, AXES, 4, seed=77)
    e.close()
    lit = shp["lit"].astype(bool)
    assert (got["EnvLit"][:, 0] == shp["lit"]).all() and lit.sum() >= 10
    six, se = shp["shape"], shp["shape_se"]
    close = lambda a, b: np.allclose(a, b, rtol=1e-8, atol=0, equal_nan=True)                           # noqa: E731
    assert close(got["EnvEnergy"][:, 0], six[:, E_] * dt) and close(got["EnvPeak"][:, 0], six[:, P_])
    assert close(got["EnvEnergy_se"][:, 0], se[:, E_] * dt) and close(got["EnvPeak_se"][:, 0], se[:, P_])
    assert close(got["EnvCentroid"][:, 0], (six[:, CEN] + 0.5) * dt) and close(got["EnvWidth"][:, 0], six[:, WID] * dt)
    assert close(got["EnvEnvelope"], shp["envelope"]) and (got["EnvEnvelope"][:, :bins[:, 0].min()] == 0).all()
    # positions: two runs differ by summation order, which moves a position only where the peak is flat to 1e-10 of itself
    pb = np.where(shp["peak_bin"] == NO_BIN, np.nan, shp["peak_bin"].astype(float))
    agree = np.nan_to_num(got["EnvPeakBin"][:, 0], nan=-1.0) == np.nan_to_num(pb, nan=-1.0)
    assert agree.mean() >= 0.9
    assert np.allclose(got["EnvPeakTime"][agree, 0], (six[agree, TP] + 0.5) * dt, rtol=0, atol=1e-6, equal_nan=True)
    # the file's numbers against the file's own (6-digit) traces: arraymatrix.m's row, smoothed four times
    checked = 0
    for i in np.flatnonzero(lit)[:8]:
        seis = read_octave(env / f"seis_{48 + i:03d}.octv")
        row = seis["TraceXYZ"].sum(axis=1)[bins[i, 0]:bins[i, 1]]
        u = row.copy()
        for _ in range(4):
            s = u.copy()
            s[1:-1] = 0.25 * u[:-2] + 0.5 * u[1:-1] + 0.25 * u[2:]
            s[0], s[-1] = 0.75 * u[0] + 0.25 * u[1], 0.75 * u[-1] + 0.25 * u[-2]
            u = s
        kk = np.arange(len(u))
        assert got["EnvEnergy"][i, 0] == pytest.approx(u.sum() * dt, rel=1e-5) and got["EnvPeak"][i, 0] == pytest.approx(u.max(), rel=1e-5)
        c = (kk * u).sum() / u.sum()
        assert got["EnvCentroid"][i, 0] == pytest.approx((c + 0.5) * dt, rel=1e-4)
        assert got["EnvWidth"][i, 0] == pytest.approx(math.sqrt((((kk - c) ** 2) * u).sum() / u.sum()) * dt, rel=1e-4)
        assert np.isfinite(got["EnvCentroid_se"][i, 0]) and got["EnvCentroid_se"][i, 0] >= 0
        checked += 1
    assert checked >= 1
