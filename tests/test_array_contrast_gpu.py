"""The contrast of two runs along a receiver array with jackknife errors on the GPU: the kernels (r3d_array_contrast) against the
host build of the lines they run, bit for bit; the known answers on the device; the run that does all of it where both runs'
blocks lie (r3d_run_batched_contrast); and ./main --array-contrast end to end."""
import ctypes as C
import itertools
import math
import subprocess

import numpy as np
import pytest
import torch

from array_image_cases import WEIGHTS
from contrast_cases import (ARRAYS, BATCH_PAIRS, F64, FIRST, N_BINS, NAMES, NAN_BITS, NEED_LOO, ONLY_X, REGIONS, RHO, SCALES, SMOOTH,
                            WINDOWS, as_case, bits, case_regions, case_windows, host_array_contrast, host_decibel, planted_blocks,
                            rows_as_blocks, same_bits, two_runs)
from cli_support import main_exe
from octave_text import read_octave
from radiative3d_amd import Engine, Model, _ffi, array_contrast
from radiative3d_amd.model import contrast_spec
from test_array_contrast import check_known, known_rows
from tests.configs import halfspace

pytestmark = pytest.mark.gpu

GUARD = 64


def run_kernel(xa, xb, first, last, weights, bins=None, regions=(), gain=None, scale=(1.0, 1.0), smooth=0, ask=NAMES):
    """r3d_array_contrast into guarded outputs, twice: the outputs as numpy, after the checks that belong to every launch -- the
    second run has the first one's bits, both sides' blocks, the bins and the gains are unchanged, the guards behind every output
    stand, an output that was not asked for (not in `ask`, or one that needs the leave-one-out rows with a B < 2) is untouched."""
    L = _ffi.hip_lib()
    Ba, S, n_bins = xa.shape[:3]
    Bb, A = xb.shape[0], last - first + 1
    b, r, g = as_case(A, bins, regions, gain)
    W, R = b.shape[1], r.shape[0]
    ins = [torch.from_numpy(np.ascontiguousarray(xa)).cuda(), torch.from_numpy(np.ascontiguousarray(xb)).cuda(),
           torch.from_numpy(b.view(np.int32)).cuda(), torch.from_numpy(g).cuda()]
    keep = [t.clone() for t in ins]
    sizes = dict(contrast=A * n_bins, contrast_se=A * n_bins, lit=A, window=A * W * 3, window_se=A * W * 3, region=R * W * 3,
                 region_se=R * W * 3, region_loo=R * W * (Ba + Bb), bad=1)
    asked = {name: name in ask and not (name in NEED_LOO and (Ba < 2 or Bb < 2)) for name in sizes}
    outs = []
    for _ in range(2):
        t = {}
        for name, n in sizes.items():
            if name in F64:
                t[name] = torch.full((n + GUARD,), -7.0, dtype=torch.float64, device="cuda")
            else:
                t[name] = torch.full((n + GUARD,), -7, dtype=torch.int64 if name == "bad" else torch.int32, device="cuda")
        spec = contrast_spec(S, n_bins, first, last, weights, ins[2].data_ptr() if W else None, ins[3].data_ptr(), W, [tuple(v) for v in r],
                             scale, smooth)
        rc = L.r3d_array_contrast(0, Ba, ins[0].data_ptr(), Bb, ins[1].data_ptr(), C.byref(spec),
                                  *[t[name].data_ptr() if asked[name] else None for name in NAMES], torch.cuda.current_stream().cuda_stream)
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
    for t, k in zip(ins, keep):
        assert torch.equal(t.view(torch.int64) if t.dtype == torch.float64 else t, k.view(torch.int64) if k.dtype == torch.float64 else k)
    for name in sizes:
        if outs[0][name] is not None:
            same = bits(outs[0][name]) == bits(outs[1][name]) if name in F64 else outs[0][name] == outs[1][name]
            assert same.all(), name
    return outs[0]


def check_against_host(xa, xb, first, last, weights, bins, regions, gain, scale, smooth, what, **kw):
    got = run_kernel(xa, xb, first, last, weights, bins, regions, gain, scale, smooth, **kw)
    want = host_array_contrast(xa, xb, first, last, weights, bins, regions, gain, scale, smooth)
    try:
        same_bits({n: (None if v is None else (int(v[0]) if n == "bad" else v)) for n, v in got.items()},
                  {n: (want[n] if got[n] is not None else None) for n in got})
    except AssertionError as e:
        raise AssertionError((what,) + e.args) from None
    return got, want


# ---- the kernels alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", N_BINS)
def test_contrast_kernels_equal_the_host_build_bit_for_bit(n_bins):
    """Every n_bins around the 64-lane tile and the strands, crossed with the batch pairs (equal, either side the larger, 64
    against 2), A (three receivers hold a blocked and a dead one), W, R, the smoothing counts and the three weight sets, each
    with its own pair of scales."""
    rng = np.random.default_rng(15000 + n_bins)
    runs = {pair: two_runs(*pair, n_bins, rng) for pair in BATCH_PAIRS}
    gains = {A: rng.uniform(0.5, 2.0, A) for A in ARRAYS}
    for (Ba, Bb), A, W, R, smooth, k in itertools.product(BATCH_PAIRS, ARRAYS, WINDOWS, REGIONS, SMOOTH, range(3)):
        if R and not W:
            continue
        xa, xb = runs[Ba, Bb]
        got, want = check_against_host(xa, xb, FIRST, FIRST + A - 1, WEIGHTS[k], case_windows(A, W, n_bins), case_regions(A, R), gains[A],
                                       SCALES[k], smooth, (n_bins, Ba, Bb, A, W, R, smooth, k))
        assert want["bad"] == 0 and want["lit"][0] == 1


def test_more_work_than_the_capped_grids_take_at_once():
    """5000 bins are 79 tiles and 20 strides of the pixel loop; 600 receivers are more than the launch has workgroups."""
    rng = np.random.default_rng(15100)
    n_bins, A = 5000, 2
    xa, xb = rng.lognormal(0.0, 1.0, (2, A, n_bins, 5)), rng.lognormal(0.0, 1.0, (2, A, n_bins, 5))
    bins = np.array([[[0, n_bins], [100, 4000]], [[3, 4999], [64, 64 * 70]]], dtype=np.uint32)
    got, _ = check_against_host(xa, xb, 0, A - 1, WEIGHTS[0], bins, [(0, 1)], [1.0, 2.0], (1.0, 0.5), 3, "5000 bins")
    assert np.isfinite(got["region_se"]).all() and (got["contrast_se"] > 0).all()
    n_bins, A = 65, 600
    xa, xb = rng.lognormal(0.0, 1.0, (2, A + 1, n_bins, 5)), rng.lognormal(0.0, 1.0, (3, A + 1, n_bins, 5))
    bins = np.tile(np.array([[0, n_bins], [5, 64]], dtype=np.uint32), (A, 1, 1))
    check_against_host(xa, xb, 1, A, WEIGHTS[2], bins, [(0, A - 1), (512, 599), (7, 7)], rng.uniform(0.5, 2.0, A), (1.0, 1.5), 2,
                       "600 receivers")


def test_bad_and_empty_windows():
    rng = np.random.default_rng(15200)
    n_bins, A = 130, 3
    xa, xb = two_runs(3, 2, n_bins, rng)
    bins = np.array([[[5, 5], [0, n_bins], [9, 3], [0, n_bins + 1]]] * A, dtype=np.uint32)
    bins[2, 1] = (n_bins, n_bins - 1)
    got, _ = check_against_host(xa, xb, FIRST, FIRST + A - 1, WEIGHTS[0], bins, [(0, 2), (0, 0)], np.ones(A), (1.0, 1.0), 2, "bad")
    assert int(got["bad"][0]) == 7
    w, wse = got["window"].reshape(A, 4, 3), got["window_se"].reshape(A, 4, 3)
    assert (bits(w[:, [0, 2, 3], RHO]) == NAN_BITS).all() and (bits(w[:, [0, 2, 3], :2]) == 0).all()        # empty and dead: no energy
    assert (bits(wse[:, [0, 2, 3], RHO]) == NAN_BITS).all() and (bits(wse[:, [0, 2, 3], :2]) == 0).all()
    assert np.isfinite(w[0, 1]).all() and np.isfinite(wse[0, 1]).all() and w[1, 1, RHO] == 0.0 and bits(w[2, 1, RHO]) == NAN_BITS
    reg = got["region"].reshape(2, 4, 3)
    assert (bits(reg[:, [0, 2, 3], RHO]) == NAN_BITS).all() and np.isfinite(reg[:, 1]).all()
    got, _ = check_against_host(xa, xb, FIRST, FIRST + A - 1, WEIGHTS[0], None, (), None, (1.0, 1.0), 0, "no window")
    assert got["window"].size == 0 and int(got["bad"][0]) == 0


def test_outputs_that_are_not_asked_for_are_not_touched():
    rng = np.random.default_rng(15300)
    n_bins, A = 129, 3
    xa, xb = two_runs(3, 4, n_bins, rng)
    args = (xa, xb, FIRST, FIRST + A - 1, WEIGHTS[2], case_windows(A, 3, n_bins), case_regions(A, 2), rng.uniform(0.5, 2.0, A), (1.0, 1.25), 2)
    full, _ = check_against_host(*args, "all")
    for ask in (("contrast",), ("contrast", "contrast_se"), ("contrast", "lit", "bad"), ("contrast", "window"), ("contrast", "window_se"),
                ("contrast", "region"), ("contrast", "region_se"), ("contrast", "region_loo"), ("contrast", "region", "window_se", "lit")):
        got, _ = check_against_host(*args, ask, ask=ask)
        assert (bits(got["contrast"]) == bits(full["contrast"])).all()


def test_receivers_whose_offset_passes_2_to_31_doubles():
    """[1][S][130][5] a side with S * 650 > 2^31: the array is the last three receivers, whose bins lie past a 32-bit offset."""
    rng = np.random.default_rng(15400)
    n_bins = 130
    S = (1 << 31) // (n_bins * 5) + 7
    tail_a, tail_b = (planted_blocks(1, n_bins, rng)[:, FIRST:FIRST + 3] for _ in range(2))
    tail_b[:, 2] = tail_a[:, 0]
    xa, xb = (torch.zeros((1, S, n_bins, 5), dtype=torch.float64, device="cuda") for _ in range(2))
    xa[:, S - 3:], xb[:, S - 3:] = torch.from_numpy(tail_a).cuda(), torch.from_numpy(tail_b).cuda()
    bins, gain, regions = case_windows(3, 2, n_bins), np.array([1.0, 0.5, 2.0]), [(0, 2), (1, 2)]
    out = array_contrast(xa, xb, S - 3, S - 1, WEIGHTS[2], torch.from_numpy(bins.view(np.int32)).cuda(), regions, torch.from_numpy(gain).cuda(),
                         (1.0, 1.25), 2)
    torch.cuda.synchronize()
    want = host_array_contrast(tail_a, tail_b, 0, 2, WEIGHTS[2], bins, regions, gain, (1.0, 1.25), 2)
    same_bits({n: (None if v is None else (v.cpu().numpy() if n != "bad" else int(v[0]))) for n, v in out.items()}, want)
    assert want["lit"].tolist() == [1, 1, 1] and (want["region"] > 0).all()


def test_refusals_enqueue_nothing():
    L = _ffi.hip_lib()
    xa = torch.full((2, 5, 40, 5), 1.5, dtype=torch.float64, device="cuda")
    xb = torch.full((3, 5, 40, 5), 0.5, dtype=torch.float64, device="cuda")
    bins = torch.tensor([[[0, 40], [3, 30]]] * 3, dtype=torch.int32, device="cuda")
    g = torch.ones(3, dtype=torch.float64, device="cuda")
    out = {n: torch.full((3 * 40,), -7.0, dtype=torch.float64, device="cuda") for n in F64}
    ints = {n: torch.full((8,), -7, dtype=torch.int64, device="cuda") for n in ("lit", "bad")}

    def call(Ba=2, Bb=3, base=xa.data_ptr(), test=xb.data_ptr(), contrast=out["contrast"].data_ptr(), se="all", spec="spec", **kw):
        s = contrast_spec(5, kw.pop("n_bins", 40), kw.pop("first", 1), kw.pop("last", 3), kw.pop("weights", (1, 1, 1, 0, 0)),
                          kw.pop("bins", bins.data_ptr()), kw.pop("g", g.data_ptr()), kw.pop("W", 2), kw.pop("regions", [(0, 2), (1, 1)]),
                          kw.pop("scale", (1.0, 1.0)), kw.pop("smooth", 2))
        for key, v in kw.items():
            setattr(s, key, v)
        opt = {n: (out[n].data_ptr() if se in ("all", n) else None) for n in NEED_LOO}
        return L.r3d_array_contrast(0, Ba, base, Bb, test, C.byref(s) if spec else None, contrast, opt["contrast_se"], ints["lit"].data_ptr(),
                                    out["window"].data_ptr(), opt["window_se"], out["region"].data_ptr(), opt["region_se"],
                                    opt["region_loo"], ints["bad"].data_ptr(), None)

    refused = [dict(base=None), dict(test=None), dict(spec=None), dict(contrast=None), dict(size=4), dict(Ba=0), dict(Bb=0), dict(Ba=65),
               dict(Bb=65), dict(n_bins=0), dict(first=3, last=2), dict(last=5), dict(weights=(1, -1, 1, 0, 0)),
               dict(weights=(math.nan, 1, 1, 0, 0)), dict(weights=(math.inf, 1, 1, 0, 0)), dict(scale=(0.0, 1.0)), dict(scale=(1.0, -2.0)),
               dict(scale=(math.inf, 1.0)), dict(scale=(1.0, math.nan)), dict(smooth=65), dict(W=9), dict(n_regions=9), dict(bins=None),
               dict(g=None), dict(W=0), dict(regions=[(0, 3)]), dict(regions=[(2, 1)]), dict(regions=[(0, 2), (3, 3)]),
               dict(Ba=1), dict(Bb=1), dict(Ba=1, se="contrast_se"), dict(Bb=1, se="window_se"), dict(Ba=1, se="region_se"),
               dict(Bb=1, se="region_loo")]
    for kw in refused:
        assert call(**dict(kw)) != 0, kw
        assert L.r3d_last_error().decode().startswith("r3d_array_contrast: "), kw
    torch.cuda.synchronize()
    assert all((t == -7.0).all() for t in out.values()) and all((t == -7).all() for t in ints.values())
    assert call() == 0 and call(Ba=1, Bb=1, se=None) == 0 and call(W=0, bins=None, g=None, regions=[]) == 0     # and these go through
    torch.cuda.synchronize()
    assert (out["contrast"] == -1.0 / 3.0).all() and int(ints["bad"][0]) == 0 and (ints["lit"].view(torch.int32)[:3] == 1).all()


# ---- known answers on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 2, 4))
def test_known_answers_on_the_device(B):
    rng = np.random.default_rng(14200)
    n_bins = 70
    base, test = known_rows(n_bins, rng)
    xa, xb = rows_as_blocks(np.repeat(base[None] / 4, B, axis=0)), rows_as_blocks(np.repeat(test[None] / 4, B, axis=0))
    got = run_kernel(xa, xb, 0, 3, ONLY_X, np.tile(np.array([[0, n_bins], [7, 66]], dtype=np.uint32), (4, 1, 1)), [(0, 0), (1, 1)], np.ones(4))
    shaped = dict(contrast=(4, n_bins), contrast_se=(4, n_bins), window=(4, 2, 3), window_se=(4, 2, 3), region=(2, 2, 3), region_se=(2, 2, 3),
                  region_loo=(2, 2, 2 * B))
    got = {n: (v.reshape(shaped[n]) if n in shaped and v is not None else v) for n, v in got.items()}
    got["bad"] = int(got["bad"][0])
    check_known(got, B)


# ---- the run that does it all ---------------------------------------------------------------------------------------------
AXES = (1.0, 1.0, 1.0, 0.0, 0.0)
N, BA_RUN, BB_RUN, SEED_A, SEED_B = 3000, 4, 3, 0x5EED, 0xBEE5
FIRST_RUN, LAST_RUN = 48, 95                      # the second of the model's three lines of 48 receivers


def lossy(args):
    """The same arguments with both layers' Q changed from 1000 to 100 (--model-args)."""
    out = [a.replace("1000", "100") if a.startswith("--model-args=") else a for a in args]
    assert out != list(args)
    return out


def run_case(model):
    A = LAST_RUN - FIRST_RUN + 1
    n_bins = model.n_bins
    bins = np.array([[[0, n_bins], [min(n_bins // 8 + i, n_bins // 2), n_bins // 2]] for i in range(A)], dtype=np.uint32)
    return bins, (np.arange(A) + 1.0) / A, [(0, A - 1), (A // 2, A - 1)]


def test_run_batched_contrast_has_the_bits_of_two_run_batched_and_of_the_call_on_the_kept_blocks(models):
    """r3d_run_batched_contrast against r3d_run_batched of either engine for the same histories and r3d_array_contrast on the
    blocks r3d_run_device_batched keeps for the same ids and seeds, bit for bit; how many entries differ is printed before
    anything is asserted.  (The engine sums a bin by atomic adds: two runs of the same histories are the same bits only as long as
    no bin's additions change their order between the runs.)  Then the refusals, which touch nothing.  No physical value of rho
    is asserted: nobody has measured one."""
    args = halfspace(3)
    ea, eb = Engine(models("halfspace", 3), reproducible=True), Engine(Model(lossy(args)), reproducible=True)
    try:
        m = ea.model
        S, n_bins = m.n_seismometers, m.n_bins
        bins, gain, regions = run_case(m)
        plain_a, plain_b = ea.run_batched(N, BA_RUN, seed=SEED_A), eb.run_batched(N, BB_RUN, seed=SEED_B)
        be_a, be_b = ea.run_batched(N, BA_RUN, seed=SEED_A, keep_batches=True)[3], eb.run_batched(N, BB_RUN, seed=SEED_B, keep_batches=True)[3]
        want = array_contrast(torch.from_numpy(be_a).cuda(), torch.from_numpy(be_b).cuda(), FIRST_RUN, LAST_RUN, AXES,
                              torch.from_numpy(bins.view(np.int32)).cuda(), regions, torch.from_numpy(gain).cuda(), (1.0, 1.0), 2)
        torch.cuda.synchronize()
        want = {n: v.cpu().numpy() for n, v in want.items()}
        side_a, side_b, got = ea.run_batched_contrast(eb, N, N, BA_RUN, BB_RUN, FIRST_RUN, LAST_RUN, AXES, bins, regions, gain, None, 2,
                                                      seed=SEED_A, other_seed=SEED_B)
        for name in F64:
            print(f"{name}: {int((bits(got[name]) != bits(want[name])).sum())} of {got[name].size} entries differ in their bits")
        for what, (res, ese, cse), (res0, ese0, cse0) in (("base", side_a, plain_a), ("test", side_b, plain_b)):
            print(f"{what}: energy {int((bits(res.energy) != bits(res0.energy)).sum())}, energy_se {int((bits(ese) != bits(ese0)).sum())} "
                  f"of {ese.size} entries differ in their bits")
        assert (got["lit"] == want["lit"].view(np.uint32)).all() and got["lit"].any()
        assert np.isfinite(want["region"][0, 0]).all() and np.isfinite(want["region_se"][0, 0]).all() and (want["contrast_se"] > 0).any()
        for name in F64:
            assert (bits(got[name]) == bits(want[name])).all(), name
        for (res, ese, cse), (res0, ese0, cse0) in ((side_a, plain_a), (side_b, plain_b)):
            assert (res.counts == res0.counts).all() and (res.scalars() == res0.scalars()).all()
            assert (bits(res.energy) == bits(res0.energy)).all() and (bits(ese) == bits(ese0)).all() and (bits(cse) == bits(cse0)).all()
        db, db_se = host_decibel(BA_RUN, BB_RUN, got["region"][0, 0, RHO], got["region_loo"][0, 0])
        print(f"region 0, window 0: rho {got['region'][0, 0, RHO]:.4f} +- {got['region_se'][0, 0, RHO]:.4f}, {db:.3f} +- {db_se:.3f} dB")
        assert math.isfinite(db) and math.isfinite(db_se)

        # the same engine on both sides is allowed
        same = ea.run_batched_contrast(ea, N, N, BA_RUN, BA_RUN, FIRST_RUN, LAST_RUN, AXES, bins, regions, gain, None, 2, seed=SEED_A,
                                       other_seed=SEED_A)[2]
        print(f"base == test: {int((bits(same['contrast']) != 0).sum())} of {same['contrast'].size} contrasts are not +0.0")
        rho = same["region"][..., RHO]                              # (1 where the region holds energy, the NaN where 3000 histories left none)
        assert (bits(same["contrast"]) == 0).all() and rho[0, 0] == 1.0 and ((rho == 1.0) | (bits(rho) == NAN_BITS)).all()

        # refusals touch nothing
        L = _ffi.hip_lib()
        hold = {n: np.full_like(v, 7) for n, v in got.items()}
        out = _ffi.ContrastResult(size=C.sizeof(_ffi.ContrastResult), **{n: v.ctypes.data for n, v in hold.items()})
        ra, rb = m.new_result(), m.new_result()
        ca, cb = ra._as_c(), rb._as_c()
        ese = np.full(ra.energy.shape, 7.0)
        bad_gain, bad_bins = gain.copy(), bins.copy()
        bad_gain[1], bad_bins[5, 1] = 0.0, (5, n_bins + 1)
        small = Engine(models("halfspace_one", 3), reproducible=True)             # (one receiver: another n_seismometers)
        try:
            cases = [dict(gain=bad_gain), dict(bins=bad_bins), dict(n_bins=n_bins + 1), dict(Ba=1), dict(Bb=1), dict(Ba=65), dict(size=8),
                     dict(contrast=None), dict(res=None), dict(test=small._e), dict(n_a=2), dict(regions=[(0, LAST_RUN - FIRST_RUN + 1)]),
                     dict(scale=(1.0, 0.0)), dict(W=9)]
            for kw in cases:
                a = dict(gain=gain, bins=bins, n_bins=n_bins, Ba=BA_RUN, Bb=BB_RUN, size=C.sizeof(_ffi.ContrastResult),
                         contrast=hold["contrast"].ctypes.data, res="res", test=eb._e, n_a=N, regions=regions, scale=(1.0, 1.0), W=2)
                a.update(kw)
                spec = contrast_spec(S, a["n_bins"], FIRST_RUN, LAST_RUN, AXES, a["bins"].ctypes.data, a["gain"].ctypes.data, a["W"],
                                     a["regions"], a["scale"], 2)
                out.size, out.contrast = a["size"], a["contrast"]
                rc = L.r3d_run_batched_contrast(ea._e, a["test"], a["n_a"], N, 0, SEED_A, SEED_B, a["Ba"], a["Bb"], C.byref(ca), C.byref(cb),
                                                ese.ctypes.data_as(_ffi._dp), None, None, None, C.byref(spec),
                                                C.byref(out) if a["res"] else None)
                assert rc != 0 and L.r3d_last_error().decode().startswith("r3d_run_batched_contrast: "), kw
        finally:
            small.close()
        assert all((v == 7).all() for v in hold.values()) and (ra.energy == 0).all() and (rb.energy == 0).all() and (ese == 7.0).all()
    finally:
        ea.close()
        eb.close()


# ---- ./main --array-contrast ---------------------------------------------------------------------------------------------------
def test_cli_array_contrast_end_to_end(tmp_path):
    """./main --error-batches=4 --array-contrast=2 --contrast-model-args=... writes contrast.octv, whose arrays are the API path's
    -- the plan of the same arguments through r3d_run_batched_contrast on two engines, same histories and seeds -- bit for bit (17
    digits round-trip a double); seis_NNN.octv is what a run without the option writes, which writes no contrast.octv."""
    from test_array_contrast import CONTRAST, TEST_ARGS
    args = halfspace(4) + ["--num-phonons=3K", "--seed=77", "--error-batches=4"]
    for name, more in (("plain", []), ("contrast", CONTRAST)):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([main_exe()] + args + [f"--output-dir={out}"] + more, cwd=out, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert not (tmp_path / "plain" / "contrast.octv").exists()
    got = read_octave(tmp_path / "contrast" / "contrast.octv")
    names = sorted(p.name for p in (tmp_path / "plain").glob("seis_*.octv"))
    assert len(names) == 288 and names == sorted(p.name for p in (tmp_path / "contrast").glob("seis_*.octv"))
    for name in names[96:100]:                                      # (at the 6 digits of the trace files)
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "contrast" / name).read_bytes(), name
    model = Model(args + CONTRAST + ["--device-tables"])           # (./main builds a run's tables on the device: the same model)
    plan = model.contrast_plan()
    test_model = Model([a for a in args if not a.startswith("--model-args=")] + ["--model-args=" + TEST_ARGS, "--device-tables"])
    n_bins, dt = model.n_bins, model.desc.params.time_per_bin
    ea, eb = Engine(model), Engine(test_model)
    try:
        _, _, want = ea.run_batched_contrast(eb, 3000, plan["num_phonons"], 4, 4, plan["first"], plan["last"], plan["axes"] + (0.0, 0.0),
                                             plan["bins"], [tuple(v) for v in plan["regions"]], plan["gain"], None, plan["smooth"], seed=77,
                                             other_seed=plan["seed"])
    finally:
        ea.close()
        eb.close()
    assert got["NumBatches"].tolist() == [[4, 4]] and got["NumPhonons"].tolist() == [[3000, 3000]] and got["Seeds"].tolist() == [[77, 78]]
    assert got["TestModelArgs"].tolist() == [plan["test_args"]] and got["BaseModelArgs"][0, 4] == 1000.0
    assert (got["Distances"][:, 0] == plan["distances"]).all() and got["TimeWindow"].tolist() == [[0.0, n_bins * dt]]
    assert (got["WindowBins"] == plan["bins"].reshape(48, 4)).all() and (got["WindowVelocities"] == plan["velocities"]).all()
    assert (got["RegionReceivers"] == plan["regions"] + 48).all() and (got["Regions"] == plan["regions_km"]).all()
    assert got["RangePower"] == 0.5 and got["RefDistance"] == plan["r_ref"] and (got["Lit"][:, 0] == want["lit"]).all()
    pairs = [("Contrast", want["contrast"]), ("ContrastSE", want["contrast_se"])]
    for k, name in enumerate(("WindowEnergyBase", "WindowEnergyTest", "WindowRatio")):
        pairs += [(name, want["window"][..., k]), (name + "SE", want["window_se"][..., k])]
    pairs += [("RegionRatio", want["region"][..., RHO]), ("RegionRatioSE", want["region_se"][..., RHO])]
    db = np.array([[host_decibel(4, 4, want["region"][r, w, RHO], want["region_loo"][r, w]) for w in range(2)] for r in range(2)])
    pairs += [("RegionDecibel", db[..., 0]), ("RegionDecibelSE", db[..., 1])]
    for name, w in pairs:
        print(f"{name}: {int((bits(got[name]) != bits(w)).sum())} of {w.size} entries differ in their bits")
    for name, w in pairs:
        assert (bits(got[name]) == bits(w)).all(), name
    assert want["lit"].any() and np.isfinite(got["WindowRatio"]).any()
