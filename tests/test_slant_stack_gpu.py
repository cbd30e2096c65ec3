"""The slant stack of a receiver array with jackknife errors on the GPU: the kernels (r3d_slant_stack) against the host build of
the lines they run, bit for bit; the known answers on the device; the run that does all of it where the blocks lie
(r3d_run_batched_slant_stack); and ./main --slant-stack end to end."""
import ctypes as C
import itertools
import math
import subprocess

import numpy as np
import pytest
import torch

from array_image_cases import WEIGHTS
from slant_cases import (BATCHES, COUNTS, F64, FIRST, N_BINS, NAN_BITS, ONLY_X, PMAX, PSTAR, as_case, bits, host_slant_stack,
                         mixed_shifts, noisy_blocks, planted_blocks, planted_moveout, rows_as_blocks, same_bits)
from cli_support import main_exe
from octave_text import read_octave
from radiative3d_amd import Engine, Model, _ffi, slant_shifts, slant_stack
from radiative3d_amd.model import slant_spec
from tests.configs import halfspace

pytestmark = pytest.mark.gpu

GUARD = 64
NAMES = ("stack", "stack_se", "fold", "power", "power_se", "picks", "picks_se", "bad", "bad_shifts")   # the call's order


def run_kernel(x, first, last, weights, shift_bin, shift_frac, gain, windows, p0=0.0, dp=0.0, smooth=0, amplitude=1, ask=NAMES):
    """r3d_slant_stack into guarded outputs, twice: the outputs as numpy, after the checks that belong to every launch -- the
    second run has the first one's bits, the blocks, the shifts, the gains and the windows are unchanged, the guards behind
    every output stand, an output that was not asked for (not in `ask`, or an se with B < 2) is untouched."""
    L = _ffi.hip_lib()
    B, S, n_bins = x.shape[:3]
    k, f, g, win = as_case(shift_bin, shift_frac, gain, windows)
    M, W = k.shape[0], win.shape[0]
    dx = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ins = [torch.from_numpy(k).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(g).cuda(),
           torch.from_numpy(win.view(np.int32).reshape(W, 2)).cuda()]
    keep = [dx.clone()] + [t.clone() for t in ins]
    sizes = dict(stack=M * n_bins, stack_se=M * n_bins, fold=M * n_bins, power=W * M, power_se=W * M, picks=W * 4, picks_se=W * 4,
                 bad=1, bad_shifts=1)
    asked = {name: name in ask and not (name.endswith("_se") and B < 2) for name in sizes}
    outs = []
    for _ in range(2):
        t = {}
        for name, n in sizes.items():
            if name in F64:
                t[name] = torch.full((n + GUARD,), -7.0, dtype=torch.float64, device="cuda")
            else:
                t[name] = torch.full((n + GUARD,), -7, dtype=torch.int64 if name in COUNTS else torch.int32, device="cuda")
        spec = slant_spec(S, n_bins, first, last, weights, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(),
                          ins[3].data_ptr() if W else None, M, W, p0, dp, smooth, amplitude)
        rc = L.r3d_slant_stack(0, B, dx.data_ptr(), C.byref(spec), *[t[name].data_ptr() if asked[name] else None for name in NAMES],
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
    assert by_bits(dx, keep[0]) and torch.equal(ins[0], keep[1]) and by_bits(ins[1], keep[2]) and by_bits(ins[2], keep[3])
    assert torch.equal(ins[3], keep[4])
    for name in sizes:
        if outs[0][name] is not None:
            same = bits(outs[0][name]) == bits(outs[1][name]) if name in F64 else outs[0][name] == outs[1][name]
            assert same.all(), name
    return outs[0]


def check_against_host(x, first, last, weights, k, f, gain, windows, p0, dp, smooth, amplitude, what, **kw):
    got = run_kernel(x, first, last, weights, k, f, gain, windows, p0, dp, smooth, amplitude, **kw)
    want = host_slant_stack(x, first, last, weights, k, f, gain, windows, p0, dp, smooth, amplitude)
    try:
        same_bits({n: (None if v is None else (int(v[0]) if n in COUNTS else v)) for n, v in got.items()},
                  {n: (want[n] if got[n] is not None else None) for n in got})
    except AssertionError as e:
        raise AssertionError((what,) + e.args) from None
    return got, want


# ---- the kernels alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", N_BINS)
def test_slant_stack_kernels_equal_the_host_build_bit_for_bit(n_bins):
    """Every n_bins around the 64-lane tile and the strands, crossed with every B, A (three receivers hold a zero one), M, W,
    smoothing count, amplitudes and energies, and the three weight sets; the shifts mix k < 0, k > 0, f == 0, f != 0 and
    receivers shifted wholly out."""
    rng = np.random.default_rng(13000 + n_bins)
    blocks = {B: planted_blocks(B, n_bins, rng) for B in BATCHES}
    shifts = {(M, A): mixed_shifts(M, A, n_bins, rng) for M in (1, 5) for A in (1, 3)}
    gains = {A: rng.uniform(0.5, 2.0, A) for A in (1, 3)}
    two = [[0, n_bins], [n_bins // 3, n_bins - n_bins // 4]]
    for B, A, M, W, smooth, amp, weights in itertools.product(BATCHES, (1, 3), (1, 5), (1, 2), (0, 2), (0, 1), WEIGHTS):
        k, f = shifts[M, A]
        got, want = check_against_host(blocks[B], FIRST, FIRST + A - 1, weights, k, f, gains[A], two[:W], 0.02, 0.015, smooth, amp,
                                       (n_bins, B, A, M, W, smooth, amp, weights))
        assert want["fold"].max() <= A and want["bad_shifts"] == 0
        assert want["picks"][0, PMAX] > 0 and np.isfinite(want["picks"][0]).all()


def test_more_work_than_the_capped_grids_take_at_once():
    """M = 256 slownesses of 5000 bins: 79 delay tiles x 64 groups of four slownesses are more units than the stack launch has
    workgroups, and the se launch loops too; 600 receivers are more than the rows launch's workgroups."""
    rng = np.random.default_rng(13100)
    n_bins, A, M = 5000, 2, 256
    x = rng.lognormal(0.0, 1.0, (2, A, n_bins, 5))
    k = rng.integers(-50, 51, (M, A)).astype(np.int32)
    f = rng.integers(0, 4, (M, A)) / 4.0
    got, want = check_against_host(x, 0, A - 1, WEIGHTS[0], k, f, [1.0, 2.0], [[0, n_bins], [100, 4000]], 0.0, 0.001, 1, 1, "capped grids")
    assert np.isfinite(got["picks_se"]).all()
    n_bins, A, M = 65, 600, 2
    x = rng.lognormal(0.0, 1.0, (2, A + 1, n_bins, 5))
    k, f = mixed_shifts(M, A, n_bins, rng)
    check_against_host(x, 1, A, WEIGHTS[2], np.clip(k, -9, 9), f, rng.uniform(0.5, 2.0, A), [[0, n_bins]], 0.0, 0.1, 2, 0, "600 receivers")


def test_bad_fractions_bad_windows_and_dead_windows():
    rng = np.random.default_rng(13200)
    n_bins, A = 130, 3
    x = planted_blocks(3, n_bins, rng)
    x[:, FIRST + 2] = x[:, FIRST][:, ::-1]
    k, f = np.zeros((2, A), dtype=np.int32), np.zeros((2, A))
    f[0, 1], f[1, 2], f[1, 0] = 1.0, math.nan, -0.125
    got, _ = check_against_host(x, FIRST, FIRST + A - 1, WEIGHTS[0], k, f, np.ones(A), [[5, 5], [0, n_bins], [9, 3], [0, n_bins + 1]],
                                0.1, 0.1, 2, 1, "bad")
    assert int(got["bad"][0]) == 2 and int(got["bad_shifts"][0]) == 3
    pk = got["picks"].reshape(4, 4)
    assert (bits(pk[[0, 2, 3], 1:]) == NAN_BITS).all() and (bits(pk[[0, 2, 3], 0]) == 0).all() and np.isfinite(pk[1]).all()
    got, _ = check_against_host(x, FIRST, FIRST + A - 1, WEIGHTS[0], np.full((2, A), n_bins), np.zeros((2, A)), np.ones(A),
                                [[0, n_bins]], 0.1, 0.1, 0, 1, "all out")
    assert (got["fold"] == 0).all() and (bits(got["stack"]) == 0).all() and (bits(got["stack_se"]) == 0).all()
    got, _ = check_against_host(x, FIRST, FIRST + A - 1, WEIGHTS[0], k, np.zeros((2, A)), np.ones(A), np.zeros((0, 2)), 0.1, 0.1, 0, 1,
                                "no window")
    assert got["power"].size == 0 and int(got["bad"][0]) == 0


def test_outputs_that_are_not_asked_for_are_not_touched():
    rng = np.random.default_rng(13300)
    n_bins, A, M = 129, 3, 5
    x = planted_blocks(3, n_bins, rng)
    k, f = mixed_shifts(M, A, n_bins, rng)
    args = (x, FIRST, FIRST + A - 1, WEIGHTS[2], k, f, np.ones(A), [[0, n_bins], [3, 90]], 0.0, 0.1, 2, 1)
    full, _ = check_against_host(*args, "all")
    for ask in (("stack",), ("stack", "picks_se"), ("stack", "stack_se", "fold"), ("stack", "power", "bad"), ("stack", "picks"),
                ("stack", "power_se", "bad_shifts")):
        got, _ = check_against_host(*args, ask, ask=ask)
        assert (bits(got["stack"]) == bits(full["stack"])).all()


def test_receivers_whose_offset_passes_2_to_31_doubles():
    """[2][S][130][5] with S * 650 > 2^31: the array is the last three receivers, whose bins lie past a 32-bit offset in both
    blocks."""
    rng = np.random.default_rng(13400)
    n_bins, M = 130, 3
    S = (1 << 31) // (n_bins * 5) + 7
    tail = planted_blocks(2, n_bins, rng)[:, FIRST:FIRST + 3]
    x = torch.zeros((2, S, n_bins, 5), dtype=torch.float64, device="cuda")
    x[:, S - 3:] = torch.from_numpy(tail).cuda()
    k, f = mixed_shifts(M, 3, n_bins, rng)
    gain, windows = np.array([1.0, 0.5, 2.0]), np.array([[0, n_bins], [64, 129]], dtype=np.int32)
    out = slant_stack(x, torch.from_numpy(k).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(gain).cuda(),
                      torch.from_numpy(windows).cuda(), S - 3, S - 1, WEIGHTS[2], 0.0, 0.1, 2, 1)
    torch.cuda.synchronize()
    want = host_slant_stack(tail, 0, 2, WEIGHTS[2], k, f, gain, windows, 0.0, 0.1, 2, 1)
    same_bits({n: (v.cpu().numpy() if n not in COUNTS else int(v[0])) for n, v in out.items()}, want)
    assert (want["power"] > 0).all()


def test_refusals_enqueue_nothing():
    L = _ffi.hip_lib()
    x = torch.full((2, 5, 40, 5), 1.5, dtype=torch.float64, device="cuda")
    k = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    f = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
    g = torch.ones(3, dtype=torch.float64, device="cuda")
    win = torch.tensor([[0, 40]], dtype=torch.int32, device="cuda")
    out = {n: torch.full((2 * 40,), -7.0, dtype=torch.float64, device="cuda") for n in F64}
    ints = {n: torch.full((2 * 40,), -7, dtype=torch.int64, device="cuda") for n in ("fold", "bad", "bad_shifts")}

    def call(B=2, blocks=x.data_ptr(), stack=out["stack"].data_ptr(), se="all", spec="spec", **kw):
        s = slant_spec(5, kw.pop("n_bins", 40), kw.pop("first", 1), kw.pop("last", 3), kw.pop("weights", (1, 1, 1, 0, 0)),
                       kw.pop("k", k.data_ptr()), kw.pop("f", f.data_ptr()), kw.pop("g", g.data_ptr()), kw.pop("w", win.data_ptr()),
                       kw.pop("M", 2), kw.pop("W", 1), kw.pop("p0", 0.0), kw.pop("dp", 0.1), kw.pop("smooth", 2), kw.pop("amplitude", 1))
        for key, v in kw.items():
            setattr(s, key, v)
        ses = {n: (out[n].data_ptr() if se in ("all", n) else None) for n in ("stack_se", "power_se", "picks_se")}
        return L.r3d_slant_stack(0, B, blocks, C.byref(s) if spec else None, stack, ses["stack_se"], ints["fold"].data_ptr(),
                                 out["power"].data_ptr(), ses["power_se"], out["picks"].data_ptr(), ses["picks_se"],
                                 ints["bad"].data_ptr(), ints["bad_shifts"].data_ptr(), None)

    refused = [dict(blocks=None), dict(spec=None), dict(stack=None), dict(k=None), dict(f=None), dict(g=None), dict(w=None),
               dict(size=4), dict(B=0), dict(B=65), dict(n_bins=0), dict(first=3, last=2), dict(last=5), dict(weights=(1, -1, 1, 0, 0)),
               dict(weights=(math.nan, 1, 1, 0, 0)), dict(smooth=65), dict(amplitude=2), dict(M=0), dict(M=257), dict(W=9),
               dict(dp=math.inf), dict(B=1), dict(B=1, se="stack_se"), dict(B=1, se="power_se"), dict(B=1, se="picks_se")]
    for kw in refused:
        assert call(**dict(kw)) != 0, kw
        assert L.r3d_last_error().decode().startswith("r3d_slant_stack: "), kw
    torch.cuda.synchronize()
    assert all((t == -7.0).all() for t in out.values()) and all((t == -7).all() for t in ints.values())
    assert call() == 0 and call(B=1, se=None) == 0 and call(W=0, w=None) == 0                          # and these go through
    torch.cuda.synchronize()
    assert (out["stack"][:80] > 0).all() and int(ints["bad"][0]) == 0


# ---- known answers on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 2, 4))
def test_planted_moveout_and_zero_se_on_the_device(B):
    p = planted_moveout()
    k, f = slant_shifts(p["dt"], p["r"], p["r_ref"], p["p0"], p["dp"], p["M"])
    x = rows_as_blocks(np.repeat(p["rows"] / B, B, axis=0))
    got = run_kernel(x, 0, 3, ONLY_X, k, f, p["gain"], p["windows"], p["p0"], p["dp"], 0, 1)
    stack, fold = got["stack"].reshape(5, 70), got["fold"].reshape(5, 70)
    assert stack[2, 20] == 2.0 and fold[2, 20] == 4 and got["power"].tolist() == [1.0, 0.75, 4.0, 0.75, got["power"][4]]
    assert got["picks"].tolist() == [4.0, 0.25, 20.0, 2.0]
    for name in ("stack_se", "power_se", "picks_se"):
        assert (got[name] is None) if B == 1 else (bits(got[name]) == 0).all(), name


# ---- the run that does it all ---------------------------------------------------------------------------------------------
AXES = (1.0, 1.0, 1.0, 0.0, 0.0)
N, B_RUN, SEED = 3000, 4, 0x5EED


FIRST_RUN, LAST_RUN = 48, 95                      # the second of the model's three lines of 48 receivers: 0 .. 260 km along x


def run_case(model):
    """The shifts, gains and windows of the run test: slownesses 0 .. 0.35 s/km over the line's receivers."""
    n_bins, dt = model.n_bins, model.desc.params.time_per_bin
    r = 260.0 * np.arange(LAST_RUN - FIRST_RUN + 1) / (LAST_RUN - FIRST_RUN)
    k, f = slant_shifts(dt, r, 0.5 * (r[0] + r[-1]), 0.0, 0.05, 8)
    gain = (r + 1.0) / (r[-1] + 1.0)
    return k, f, gain, np.array([[0, n_bins], [n_bins // 4, n_bins // 2]], dtype=np.uint32)


def test_run_batched_slant_stack_has_the_bits_of_run_batched_and_of_the_call_on_the_kept_blocks(models):
    """r3d_run_batched_slant_stack against r3d_run_batched of the same histories and r3d_slant_stack on the blocks
    r3d_run_device_batched keeps for the same ids and seed, bit for bit; how many entries differ is printed before anything is
    asserted.  (The engine sums a bin by atomic adds: two runs of the same histories are the same bits only as long as no bin's
    additions change their order between the runs.)  Then the refusals, which touch nothing."""
    e = Engine(models("halfspace", 3), reproducible=True)
    try:
        m = e.model
        S, n_bins = m.n_seismometers, m.n_bins
        k, f, gain, windows = run_case(m)
        res0, ese0, cse0 = e.run_batched(N, B_RUN, seed=SEED)
        _, _, _, be, _ = e.run_batched(N, B_RUN, seed=SEED, keep_batches=True)
        want = slant_stack(torch.from_numpy(be).cuda(), torch.from_numpy(k).cuda(), torch.from_numpy(f).cuda(),
                           torch.from_numpy(gain).cuda(), torch.from_numpy(windows.view(np.int32)).cuda(), FIRST_RUN, LAST_RUN, AXES, 0.0, 0.05, 2, 1)
        torch.cuda.synchronize()
        want = {n: v.cpu().numpy() for n, v in want.items()}
        res, ese, cse, got = e.run_batched_slant_stack(N, B_RUN, k, f, gain, windows, FIRST_RUN, LAST_RUN, AXES, 0.0, 0.05, 2, 1, seed=SEED)
        for name in F64:
            print(f"{name}: {int((bits(got[name]) != bits(want[name])).sum())} of {got[name].size} entries differ in their bits")
        print(f"energy: {int((bits(res.energy) != bits(res0.energy)).sum())}, energy_se: {int((bits(ese) != bits(ese0)).sum())} "
              f"of {ese.size} entries differ in their bits")
        assert (got["fold"] == want["fold"].view(np.uint32)).all() and want["fold"].max() == LAST_RUN - FIRST_RUN + 1
        assert (want["power"][0] > 0).all() and np.isfinite(want["picks"][0]).all() and np.isfinite(want["picks_se"][0]).all()
        for name in F64:
            assert (bits(got[name]) == bits(want[name])).all(), name
        assert (res.counts == res0.counts).all() and (res.scalars() == res0.scalars()).all()
        assert (bits(res.energy) == bits(res0.energy)).all() and (bits(ese) == bits(ese0)).all() and (bits(cse) == bits(cse0)).all()

        # refusals touch nothing
        L = _ffi.hip_lib()
        hold = {n: np.full_like(v, 7) for n, v in got.items()}
        out = _ffi.SlantResult(size=C.sizeof(_ffi.SlantResult), **{n: v.ctypes.data for n, v in hold.items()})
        r = m.new_result()
        rc_ = r._as_c()
        before = r.energy.copy()
        bad_gain, bad_f, bad_win = gain.copy(), f.copy(), windows.copy()
        bad_gain[1], bad_f[2, 3], bad_win[1] = -1.0, 1.0, (5, n_bins + 1)
        cases = [dict(gain=bad_gain), dict(f=bad_f), dict(windows=bad_win), dict(n_bins=n_bins + 1), dict(B=1), dict(B=65), dict(size=8),
                 dict(M=0), dict(stack=None)]
        for kw in cases:
            a = dict(gain=gain, f=f, windows=windows, n_bins=n_bins, B=B_RUN, size=C.sizeof(_ffi.SlantResult), M=8, stack=hold["stack"].ctypes.data)
            a.update(kw)
            spec = slant_spec(S, a["n_bins"], FIRST_RUN, LAST_RUN, AXES, k.ctypes.data, a["f"].ctypes.data, a["gain"].ctypes.data,
                              a["windows"].ctypes.data, a["M"], 2, 0.0, 0.05, 2, 1)
            out.size, out.stack = a["size"], a["stack"]
            rc = L.r3d_run_batched_slant_stack(e._e, N, 0, SEED, a["B"], C.byref(rc_), None, None, C.byref(spec), C.byref(out))
            assert rc != 0 and L.r3d_last_error().decode().startswith("r3d_run_batched_slant_stack: "), kw
        assert all((v == 7).all() for v in hold.values()) and (r.energy == before).all()
    finally:
        e.close()


# ---- ./main --slant-stack ------------------------------------------------------------------------------------------------------
def test_cli_slant_stack_end_to_end(tmp_path):
    """./main --error-batches=4 --slant-stack=... writes slantstack.octv, whose arrays are the API path's -- the plan of the same
    arguments through r3d_run_batched_slant_stack, same histories and seed -- bit for bit (17 digits round-trip a double), p* in
    s/km and tau* in seconds; seis_NNN.octv is what a run without the option writes."""
    args = halfspace(4) + ["--num-phonons=3K", "--seed=77", "--error-batches=4"]
    slant = ["--slant-stack=0,0.35,8,nan,2", "--slant-array=48,95", "--slant-axes=1,1,0", "--slant-range-power=0.5",
             "--slant-windows=0,200,20,90"]
    for name, more in (("plain", []), ("slant", slant)):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([main_exe()] + args + [f"--output-dir={out}"] + more, cwd=out, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert not (tmp_path / "plain" / "slantstack.octv").exists()
    got = read_octave(tmp_path / "slant" / "slantstack.octv")
    names = sorted(p.name for p in (tmp_path / "plain").glob("seis_*.octv"))
    assert len(names) == 288 and names == sorted(p.name for p in (tmp_path / "slant").glob("seis_*.octv"))
    for name in names[96:100]:                                      # (at the 6 digits of the trace files)
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "slant" / name).read_bytes(), name
    model = Model(args + slant + ["--device-tables"])              # (./main builds a run's tables on the device: the same model)
    plan = model.slant_plan()
    n_bins, dt = model.n_bins, model.desc.params.time_per_bin
    e = Engine(model)
    try:
        _, _, _, want = e.run_batched_slant_stack(3000, 4, plan["shift_bin"], plan["shift_frac"], plan["gain"], plan["windows"], 48, 95,
                                                  (1, 1, 0, 0, 0), plan["p0"], plan["dp"], 2, 1, seed=77)
    finally:
        e.close()
    assert (got["Slowness"][:, 0] == plan["p0"] + np.arange(8) * plan["dp"]).all() and got["TimeWindow"].tolist() == [[0.0, n_bins * dt]]
    assert got["RefDistance"] == plan["r_ref"] and (got["Distances"][:, 0] == plan["distances"]).all()
    assert got["NumBatches"] == 4 and got["NumPhonons"] == 3000 and got["WindowBins"].tolist() == [[0, n_bins], [40, 180]]
    assert (got["Windows"] == got["WindowBins"] * dt).all() and (got["Fold"] == want["fold"]).all() and got["Fold"].max() == 48
    for name, key in (("Stack", "stack"), ("StackSE", "stack_se"), ("Power", "power"), ("PowerSE", "power_se")):
        print(f"{name}: {int((bits(got[name]) != bits(want[key])).sum())} of {want[key].size} entries differ in their bits")
    for name, key in (("Stack", "stack"), ("StackSE", "stack_se"), ("Power", "power"), ("PowerSE", "power_se")):
        assert (bits(got[name]) == bits(want[key])).all(), name
    scale = np.array([1.0, 1.0, dt, 1.0])
    assert (bits(got["Picks"]) == bits(want["picks"] * scale)).all() and (bits(got["PicksSE"]) == bits(want["picks_se"] * scale)).all()
    assert (got["Power"][0] > 0).all() and np.isfinite(got["Picks"][0]).all() and 0.0 <= got["Picks"][0, PSTAR] <= 0.35
