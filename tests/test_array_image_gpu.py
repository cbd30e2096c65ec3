"""The travel-time image of a receiver array with jackknife errors on the GPU: the kernel (r3d_array_image) against the host
build of the lines it runs, value for value; on the kept blocks of real batched runs; the run that does all of it where the
blocks lie (r3d_run_batched_array_image); and ./main --ttimage end to end."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest
import torch

from array_image_cases import (BATCHES, CURVE, FIRST, LEGACY, N_BINS, S_ALL, WEIGHTS, array_blocks, curve_values,
                               host_array_image, host_powerlaw, restated_image)
from batch_cases import sum_in_order
from cli_support import main_exe
from octave_text import read_octave
from radiative3d_amd import Engine, _ffi, array_image, window_sums
from radiative3d_amd.model import array_image_spec
from tests.configs import halfspace
from window_cases import host_moments

pytestmark = pytest.mark.gpu

GUARD = 64
F64 = ("image", "image_se", "row_sum", "peak")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def run_kernel(x, first, last, weights, k, mode=LEGACY, rho=0.3, curve=None, Tw=0.0):
    """r3d_array_image into guarded outputs, twice: the outputs as numpy, after the checks that belong to every launch --
    the second run has the first one's bits, the blocks are unchanged, the guards behind every output stand."""
    L = _ffi.hip_lib()
    B, S, n_bins = x.shape[:3]
    A = last - first + 1
    dx = torch.from_numpy(x).cuda()
    keep = dx.clone()
    dcurve = torch.from_numpy(np.ascontiguousarray(curve, dtype=np.float64)).cuda() if mode == CURVE else None
    sizes = dict(image=A * n_bins, image_se=A * n_bins, row_sum=B * A, peak=A, peak_bin=A, lit=A, bad=1)
    outs = []
    for _ in range(2):
        t = {}
        for name, n in sizes.items():
            if name in F64:
                t[name] = torch.full((n + GUARD,), -7.0, dtype=torch.float64, device="cuda")
            else:
                t[name] = torch.full((n + GUARD,), -7, dtype=torch.int64 if name == "bad" else torch.int32, device="cuda")
        spec = array_image_spec(S, n_bins, first, last, weights, k, rho, dcurve.data_ptr() if dcurve is not None else None, Tw)
        rc = L.r3d_array_image(0, B, dx.data_ptr(), C.byref(spec), t["image"].data_ptr(),
                               t["image_se"].data_ptr() if B >= 2 else None, t["row_sum"].data_ptr(), t["peak"].data_ptr(),
                               t["peak_bin"].data_ptr(), t["lit"].data_ptr(), t["bad"].data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.r3d_last_error().decode()
        torch.cuda.synchronize()
        got = {}
        for name, n in sizes.items():
            if name == "image_se" and B < 2:
                assert (t[name] == -7.0).all()                      # (not asked for: not touched)
                got[name] = None
                continue
            assert (t[name][n:] == -7).all(), name
            got[name] = t[name][:n].cpu().numpy()
        outs.append(got)
    assert torch.equal(dx, keep)
    for name in sizes:
        if outs[0][name] is not None:
            same = bits(outs[0][name]) == bits(outs[1][name]) if name in F64 else outs[0][name] == outs[1][name]
            assert same.all(), name
    return outs[0]


def check_against_host(x, first, last, weights, k, mode, rho, curve, Tw, what):
    got = run_kernel(x, first, last, weights, k, mode, rho, curve, Tw)
    want = host_array_image(x, first, last, weights, k, mode, rho, curve, Tw)
    for name in F64:                                                # value for value, the sign of a zero included
        if want[name] is None:
            assert got[name] is None
        else:
            assert (bits(got[name]) == bits(want[name].reshape(-1))).all(), (what, name)
    assert (got["peak_bin"] == want["peak_bin"]).all() and (got["lit"] == want["lit"]).all(), what
    assert int(got["bad"][0]) == want["bad"], what
    return got, want


# ---- the kernel alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", N_BINS)
def test_array_image_kernel_equals_the_host_build_value_for_value(n_bins):
    rng = np.random.default_rng(7000 + n_bins)
    n = 0
    for B in BATCHES:
        x = array_blocks(B, n_bins, rng)
        for A in (1, 3):
            curve = curve_values(A, rng)
            for k in (0, 1, 2):
                for mode in (LEGACY, CURVE):
                    weights, rho = WEIGHTS[n % 3], (0.0, 0.3, 1.0)[(n // 3) % 3]
                    got, want = check_against_host(x, FIRST, FIRST + A - 1, weights, k, mode, rho, curve, n_bins * 0.5,
                                                   (n_bins, B, A, k, mode))
                    n += 1
                    if A == 3:
                        assert want["lit"].tolist() == ([1, 1, 0] if mode == LEGACY else [1, 1, 1])
                        assert (bits(got["image"].reshape(3, n_bins)[2]) == 0).all()                 # the zero row: +0.0
                    if n_bins >= 3:
                        assert got["peak_bin"][0] == n_bins // 3                                      # the tie's first bin


def test_row_sums_are_window_sums_with_full_windows_on_the_same_blocks():
    rng = np.random.default_rng(7100)
    for n_bins, B in ((65, 1), (130, 3), (400, 64)):
        x = array_blocks(B, n_bins, rng)
        dx = torch.from_numpy(x).cuda()
        bins = torch.tensor([[[0, n_bins]]] * S_ALL, dtype=torch.int32, device="cuda")
        for weights in WEIGHTS:
            out = array_image(dx, FIRST, FIRST + 2, weights)
            y, _, _ = window_sums(dx, bins, weights)
            torch.cuda.synchronize()
            assert (bits(out["row_sum"].cpu().numpy()) == bits(y[:, FIRST:FIRST + 3, 0].cpu().numpy())).all()


def test_receivers_whose_offset_passes_2_to_31_doubles():
    """[2][S][130][5] with S * 650 > 2^31: the array is the last three receivers, whose bins lie past a 32-bit offset in both
    blocks (and the second block's start does too)."""
    rng = np.random.default_rng(7150)
    n_bins = 130
    S = (1 << 31) // (n_bins * 5) + 7
    tail = array_blocks(2, n_bins, rng)[:, FIRST:FIRST + 3]
    x = torch.zeros((2, S, n_bins, 5), dtype=torch.float64, device="cuda")
    x[:, S - 3:] = torch.from_numpy(tail).cuda()
    curve = curve_values(3, rng)
    for mode in (LEGACY, CURVE):
        out = array_image(x, S - 3, S - 1, WEIGHTS[2], 1, 0.3, torch.from_numpy(curve).cuda() if mode == CURVE else None, 65.0)
        torch.cuda.synchronize()
        want = host_array_image(tail, 0, 2, WEIGHTS[2], 1, mode, 0.3, curve, 65.0)
        for name in F64:
            assert (bits(out[name].cpu().numpy()) == bits(want[name])).all(), (mode, name)
        assert (out["peak_bin"].cpu().numpy() == want["peak_bin"]).all() and want["peak"][0] > 0


def test_a_bad_curve_value_is_counted_and_its_row_is_dead():
    rng = np.random.default_rng(7200)
    B, n_bins, A = 3, 130, 4
    x = array_blocks(B, n_bins, rng)
    # (the last: a curve value whose c_s / Tw underflows to zero)
    for value, Tw in ((0.0, 65.0), (-2.0, 65.0), (math.nan, 65.0), (math.inf, 65.0), (-math.inf, 65.0), (1e-320, 1e300)):
        at = int(rng.integers(0, A))
        curve = curve_values(A, rng)
        curve[at] = value
        got, want = check_against_host(x, FIRST, FIRST + A - 1, WEIGHTS[0], 1, CURVE, 0.0, curve, Tw, ("bad curve", value))
        assert int(got["bad"][0]) == 1 and got["lit"].tolist() == [int(i != at) for i in range(A)]
        assert (bits(got["image"].reshape(A, n_bins)[at]) == 0).all() and (bits(got["image_se"].reshape(A, n_bins)[at]) == 0).all()
    # LEGACY counts nothing
    assert int(run_kernel(x, FIRST, FIRST + 2, WEIGHTS[0], 1)["bad"][0]) == 0


def test_refusals_enqueue_nothing():
    L = _ffi.hip_lib()
    x = torch.full((2, 5, 40, 5), 1.5, dtype=torch.float64, device="cuda")
    curve = torch.full((3,), 2.0, dtype=torch.float64, device="cuda")
    out = {n: torch.full((2 * 3 * 40,), -7.0, dtype=torch.float64, device="cuda") for n in ("image", "se", "rows", "peak")}
    ints = {n: torch.full((8,), -7, dtype=torch.int64, device="cuda") for n in ("bin", "lit", "bad")}

    def call(B=2, blocks=x.data_ptr(), image=out["image"].data_ptr(), se=out["se"].data_ptr(), spec="spec", **kw):
        s = array_image_spec(5, kw.pop("n_bins", 40), kw.pop("first", 1), kw.pop("last", 3), kw.pop("weights", (1, 1, 1, 0, 0)),
                             kw.pop("k", 1), kw.pop("rho", 0.3), kw.pop("curve_ptr", None), kw.pop("Tw", 0.0))
        for key, v in kw.items():
            setattr(s, key, v)
        return L.r3d_array_image(0, B, blocks, C.byref(s) if spec else None, image, se, out["rows"].data_ptr(),
                                 out["peak"].data_ptr(), ints["bin"].data_ptr(), ints["lit"].data_ptr(), ints["bad"].data_ptr(),
                                 None)

    refused = [dict(blocks=None), dict(spec=None), dict(image=None), dict(size=4), dict(B=0), dict(B=65), dict(n_bins=0),
               dict(first=3, last=2), dict(last=5), dict(weights=(1, -1, 1, 0, 0)), dict(weights=(1, math.inf, 1, 0, 0)),
               dict(weights=(math.nan, 1, 1, 0, 0)), dict(k=3), dict(rho=-0.1), dict(rho=1.5), dict(rho=math.nan), dict(mode=2),
               dict(mode=_ffi.R3D_ARRAY_CURVE, Tw=20.0), dict(curve_ptr=curve.data_ptr(), Tw=0.0),
               dict(curve_ptr=curve.data_ptr(), Tw=math.inf), dict(curve_ptr=curve.data_ptr(), Tw=-1.0),
               dict(curve_ptr=curve.data_ptr(), Tw=math.nan), dict(B=1)]
    for kw in refused:
        assert call(**dict(kw)) != 0, kw
        assert L.r3d_last_error().decode().startswith("r3d_array_image: "), kw
    torch.cuda.synchronize()
    assert all((t == -7.0).all() for t in out.values()) and all((t == -7).all() for t in ints.values())
    assert call() == 0 and call(B=1, se=None) == 0 and call(curve_ptr=curve.data_ptr(), Tw=20.0) == 0   # and these go through
    torch.cuda.synchronize()
    assert (out["image"][:120] >= 0).all()


# ---- real blocks, and the run that does it all ---------------------------------------------------------------------------
AXES = (1.0, 1.0, 1.0, 0.0, 0.0)
K, RHO, GIVEN = 1, 0.3, (5.0e-3, -1.5)


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
    """name -> the kept blocks of one batched run and what r3d_array_image makes of them on the device, in both modes (the
    curve: GIVEN over the plan's range): computed once, shared, left unchanged."""
    cache = {}

    def get(name, n, B=10, seed=0x5EED):
        if name not in cache:
            e = engines(name)
            m = e.model
            S = m.n_seismometers
            dist, azi = m.ttimage_plan(dict(first=0, last=S - 1))
            X = dist[0] + np.arange(S) * ((dist[-1] - dist[0]) / (S - 1))
            curve = GIVEN[0] * np.array([math.pow(v, GIVEN[1]) for v in X])
            Tw = m.n_bins * m.desc.params.time_per_bin
            res, ese, cse, be, bc = e.run_batched(n, B, seed=seed, keep_batches=True)
            dbe = torch.from_numpy(be).cuda()
            legacy = array_image(dbe, 0, S - 1, AXES, K, RHO)
            curved = array_image(dbe, 0, S - 1, AXES, K, curve=torch.from_numpy(curve).cuda(), window_length=Tw)
            torch.cuda.synchronize()
            assert torch.equal(dbe, torch.from_numpy(be).cuda())
            cache[name] = dict(n=n, B=B, seed=seed, dist=dist, azi=azi, curve=curve, Tw=Tw, res=res, be=be,
                               legacy={k: v.cpu().numpy() for k, v in legacy.items()},
                               curved={k: v.cpu().numpy() for k, v in curved.items()})
        return cache[name]
    return get


CASES = [("halfspace", 50000), ("crustpinch", 20000)]


@pytest.mark.parametrize("name,n", CASES)
def test_image_and_errors_on_the_blocks_of_a_real_run_equal_the_host_build(composed, name, n):
    k = composed(name, n)
    S = k["be"].shape[1]
    for mode, got in ((LEGACY, k["legacy"]), (CURVE, k["curved"])):
        want = host_array_image(k["be"], 0, S - 1, AXES, K, mode, RHO, k["curve"], k["Tw"])
        for key in F64:
            assert (bits(got[key]) == bits(want[key])).all(), (name, mode, key)
        assert (got["peak_bin"] == want["peak_bin"]).all() and (got["lit"] == want["lit"]).all() and int(got["bad"][0]) == 0
    lit = k["legacy"]["lit"].astype(bool)
    print(f"{name}: {lit.sum()} of {S} rows lit")
    assert lit.any() and np.isfinite(k["legacy"]["image_se"]).all() and (k["legacy"]["image"][lit].max(axis=1) > 0).all()
    assert (k["legacy"]["image"][~lit] == 0).all()


@pytest.mark.parametrize("name,n", CASES)
def test_run_batched_array_image_equals_the_composition(engines, composed, name, n):
    """Two engine runs of the same histories differ by 1e-11 of a bin's P + S energy in each component
    (tests/test_gpu_parity.energies_agree).  With the weights (1, 1, 1, 0, 0) a bin's weighted energy moves by r = 3e-11
    PS_b / t_b of itself at most; a pixel -- a root of it over a sum or a maximum of such roots, or over a constant -- by 2 r
    to first order (asserted: 2.5 r of the pixel), and the jackknife of B such pixels by sqrt(B) times the largest such move."""
    k = composed(name, n)
    e = engines(name)
    B, be = k["B"], k["be"]
    S, n_bins = be.shape[1:3]
    res, ese, cse, img = e.run_batched_array_image(n, B, 0, S - 1, AXES, K, RHO, fit=(2, S), ranges=(k["dist"][0], k["dist"][-1]),
                                                   curve=GIVEN, seed=k["seed"], keep_row_sums=True)
    assert (res.counts == k["res"].counts).all() and (res.scalars() == k["res"].scalars()).all()
    t = sum_in_order(be)[..., :3].sum(-1)
    ps = sum_in_order(be)[..., 3:].sum(-1)
    with np.errstate(all="ignore"):
        r = np.where(t > 0, 3e-11 * ps / t, 0.0).max(axis=1, keepdims=True)
    print(f"{name}: largest relative move of a bin's weighted energy that the parity figure allows: {r.max():.3g}")
    assert r.max() < 1e-9
    # the raw row sums and their moments
    want_rows = k["legacy"]["row_sum"]
    scale = be[..., 3:].sum(axis=(2, 3))
    assert (np.abs(img["batch_row_sum"] - want_rows) <= 1e-11 * scale + 1e-300).all()
    assert (img["summed"] == sum_in_order(img["batch_row_sum"])).all()
    assert (bits(img["summed_se"]) == bits(host_moments(img["batch_row_sum"])[1])).all()
    # pixels and errors, both images
    assert img["curve_made"] and (bits(img["curve"]) == bits(k["curve"])).all()
    for mode, got, got_se, want in ((LEGACY, img["image"], img["image_se"], k["legacy"]),
                                    (CURVE, img["image_curve"], img["image_curve_se"], k["curved"])):
        assert (np.abs(got - want["image"]) <= 2.5 * r * want["image"] + 1e-300).all(), (name, mode)
        _, _, _, loo_max = restated_image(be, 0, S - 1, AXES, K, mode, RHO, k["curve"], k["Tw"])
        lim = math.sqrt(B) * 2.5 * r * loo_max.astype(np.float64) + 1e-300
        assert (np.abs(got_se - want["image_se"]) <= lim).all(), (name, mode)
    assert (img["lit"] == k["legacy"]["lit"]).all()
    assert (np.abs(img["peak"] - k["legacy"]["peak"]) <= 3e-11 * ps.max(axis=1) + 1e-300).all()
    # the peak's bin, exactly, where no other bin comes within the figure of it
    top2 = np.sort(t, axis=1)[:, -2:] if n_bins > 1 else np.stack([np.zeros(S), t[:, 0]], axis=1)
    clear = (top2[:, 1] - top2[:, 0]) > 1e-9 * top2[:, 1]
    assert clear.any() and (img["peak_bin"][clear] == k["legacy"]["peak_bin"][clear]).all()
    # the fit is the host functions' on the run's own row sums times dt (NaN where a receiver of the range caught nothing)
    dt = k["Tw"] / n_bins
    rc, lnc, q, se_c, se_q, _ = host_powerlaw(img["batch_row_sum"] * dt, k["dist"][0], k["dist"][-1], 2, S)
    want_fit = (math.exp(lnc), q, se_c, se_q)
    for g, w in zip(img["fit"] + img["fit_se"], want_fit):
        assert (math.isnan(g) and math.isnan(w)) or g == pytest.approx(w, rel=1e-12), (img["fit"], img["fit_se"], want_fit)
    # ... and the run's own results are r3d_run_batched's
    plain, pese, pcse = e.run_batched(n, B, seed=k["seed"])
    assert (plain.counts == res.counts).all() and np.allclose(pcse, cse, rtol=1e-12, atol=0)
    from tests.test_gpu_parity import energies_agree
    assert energies_agree(plain.energy, res.energy) and np.allclose(pese, ese, rtol=1e-6, atol=1e-11 * ps.max())


def test_run_batched_array_image_shares_the_batched_runs_refusals_and_touches_nothing(engines):
    e = engines("crustpinch")
    m = e.model
    L = e._lib
    S, n_bins = m.n_seismometers, m.n_bins
    A, B = S - 2, 4
    dist, _ = m.ttimage_plan(dict(first=1, last=S - 2))

    def fresh():
        res = m.new_result()
        res.energy[:], res.counts[:] = 3.5, 7
        px = (A, n_bins)
        return dict(res=res, ese=np.full(res.energy.shape, -1.0), cse=np.full(res.counts.shape, -1.0),
                    image=np.full(px, -2.0), image_se=np.full(px, -2.0), summed=np.full(A, 2.5), summed_se=np.full(A, -2.0),
                    peak=np.full(A, -2.0), peak_bin=np.full(A, 9, dtype=np.uint32), lit=np.full(A, 9, dtype=np.uint32),
                    curve=np.full(A, -2.0), image_curve=np.full(px, -2.0), image_curve_se=np.full(px, -2.0))

    def call(n, batches, bufs, fit=(2, A), curve=(math.nan, math.nan), drop=(), **spec_kw):
        spec = array_image_spec(S, n_bins, 1, S - 2, AXES, K, RHO, None, n_bins * m.desc.params.time_per_bin, fit,
                                (dist[0], dist[-1]), curve)
        for key, v in spec_kw.items():
            setattr(spec, key, v)
        out = _ffi.ArrayImageResult(size=C.sizeof(_ffi.ArrayImageResult),
                                    **{key: v.ctypes.data for key, v in bufs.items() if key not in ("res", "ese", "cse") + drop})
        c = bufs["res"]._as_c()
        rc = L.r3d_run_batched_array_image(e._e, n, 0, 0x5EED, batches, C.byref(c), bufs["ese"].ctypes.data_as(_ffi._dp),
                                           bufs["cse"].ctypes.data_as(_ffi._dp), C.byref(spec), C.byref(out))
        bufs["res"]._from_c(c)
        return rc, out

    def refused(n, batches, match, **kw):
        bufs = fresh()
        rc, _ = call(n, batches, bufs, **kw)
        assert rc != 0 and match in L.r3d_last_error().decode(), L.r3d_last_error().decode()
        r = bufs["res"]
        assert (r.energy == 3.5).all() and (r.counts == 7).all() and not r.scalars().any()
        assert (bufs["ese"] == -1.0).all() and (bufs["cse"] == -1.0).all() and (bufs["summed"] == 2.5).all()
        assert all((bufs[key] == -2.0).all() for key in ("image", "image_se", "summed_se", "peak", "curve", "image_curve",
                                                         "image_curve_se"))
        assert (bufs["peak_bin"] == 9).all() and (bufs["lit"] == 9).all()

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
    # the spec
    refused(1000, B, "not the model's", n_bins=n_bins - 1)
    refused(1000, B, "negative or not finite", weight=(C.c_double * 5)(0, 0, -1.0, 0, 0))
    refused(1000, B, "gamma_log2", gamma_log2=3)
    refused(1000, B, "rho", rho=1.25)
    refused(1000, B, "fit needs", fit=(3, A + 1))
    refused(1000, B, "fit needs", fit=(4, 4))
    refused(1000, B, "given curve needs", fit=(0, 0), curve=GIVEN)
    refused(1000, B, "not finite and > 0", curve=(-1.0, -1.5))          # made and checked on the host: refused, not counted
    refused(1000, B, "null curve", drop=("image_curve",))
    refused(1000, B, "null image", drop=("image_se",))
    with pytest.raises(RuntimeError, match="at least 2 batches"):
        e.run_batched_array_image(1000, 1, 1, S - 2, AXES)
    # with all of that gone the same call goes through: summed ADDED into, everything else WRITTEN
    bufs = fresh()
    rc, out = call(4000, B, bufs, curve=GIVEN)
    assert rc == 0, L.r3d_last_error().decode()
    plain = e.run(4000)
    assert (bufs["res"].counts - 7 == plain.counts).all()
    want = plain.energy[1:S - 1, :, :3].sum(axis=(1, 2))
    assert np.allclose(bufs["summed"] - 2.5, want, rtol=1e-9, atol=1e-12 * want.max()) and want.max() > 0
    assert (bufs["image"] >= 0).all() and (bufs["image_se"] >= 0).all() and (bufs["lit"] <= 1).all() and bufs["lit"].any()
    assert out.curve_made == 1 and (bufs["curve"] > 0).all() and (bufs["image_curve"] >= 0).all()


# ---- ./main --ttimage --------------------------------------------------------------------------------------------------------
def test_cli_ttimage_end_to_end(tmp_path):
    args = halfspace(4) + ["--num-phonons=2M", "--seed=77", "--error-batches=8"]
    plain, tt = tmp_path / "plain", tmp_path / "tt"
    plain.mkdir(), tt.mkdir()
    for out, extra in ((plain, []), (tt, ["--ttimage", "--ttimage-array=48,95", "--ttimage-fit=4,48"])):
        r = subprocess.run([main_exe()] + args + [f"--output-dir={out}"] + extra, cwd=out, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert not (plain / "ttimage.octv").exists()
    # the seis and err files are what they are without the image's options, byte for byte
    names = sorted(p.name for p in plain.glob("seis_*.octv"))
    assert len(names) == 288 and names == sorted(p.name for p in tt.glob("seis_*.octv"))
    for name in names:
        assert (plain / name).read_bytes() == (tt / name).read_bytes(), name
    got = read_octave(tt / "ttimage.octv")
    A, n_bins, dt = 48, 400, 0.5
    assert (got["TTSeismometers"][:, 0] == np.arange(48, 96)).all() and got["TTBatches"] == 8 and got["TTNumBins"] == n_bins
    assert got["TTGamma"] == 2 and got["TTNorm"] == 0.3 and got["TTAxes"].tolist() == [[1, 1, 1]]
    assert got["TTTimeWindow"].tolist() == [[0, n_bins * dt]] and got["TTFitRange"].tolist() == [[4, 48]]
    image, image_se, lit = got["TTImage"], got["TTImage_se"], got["TTLit"][:, 0].astype(bool)
    assert image.shape == (A, n_bins) and image_se.shape == (A, n_bins)
    E, peak, peak_bin = got["TTSummedEnergy"][:, 0], got["TTPeakEnergy"][:, 0], got["TTPeakBin"][:, 0].astype(int)
    dist, azi = got["TTDistances"][:, 0], got["TTAzimuths"][:, 0]
    lit_by_many = 0
    for i in range(A):
        seis = read_octave(tt / f"seis_{48 + i:03d}.octv")
        delta = seis["Location"][0, :2] - seis["EventLoc"][0, :2]
        assert abs(dist[i] - np.hypot(*delta)) <= 1e-5 * max(dist[i], 1.0)                     # range_km.m
        assert abs((azi[i] - math.degrees(math.atan2(delta[0], delta[1]))) % 360.0) <= 1e-3     # azimuth_deg.m
        # arraymatrix.m's row of this receiver from the file's own (6-digit) traces; every term is non-negative
        row = seis["TraceXYZ"].sum(axis=1)
        assert E[i] == pytest.approx(row.sum() * dt, rel=1e-5, abs=0)
        assert peak[i] == pytest.approx(row.max(), rel=1e-5, abs=0)
        assert lit[i] == (row.max() > 0)
        if not lit[i]:
            assert (image[i] == 0).all() and (image_se[i] == 0).all()
            continue
        assert row[peak_bin[i]] == pytest.approx(row.max(), rel=1e-5)
        # arrayimage.m:65-81 with gamma 2 and norm 0.3, at the energies' figure: a 6-digit value is off by 5e-6 at most, the
        # root halves that, the quotient by a sum or a maximum of such roots adds as much again: 5e-6 <= 1e-5
        g = np.sqrt(row)
        want = 0.7 * g / g.sum() + 0.3 * g / g.max()
        assert np.allclose(image[i], want, rtol=1e-5, atol=0)
        # se > 0 wherever the row is lit: with B >= 2 the leave-one-out pixels of a positive pixel differ -- also in a row
        # that ONE batch lit, whose one dead leave-one-out row gives the spread -- and a zero pixel has none
        assert (image_se[i][image[i] > 0] > 0).all(), i
        assert np.isfinite(image_se[i]).all() and (image_se[i][image[i] == 0] == 0).all()
        lit_by_many += got["TTSummedEnergy_se"][i, 0] < E[i] * (1 - 1e-9)    # (one batch alone: the sum's se is the sum)
    assert (got["TTSummedEnergy_se"][:, 0][E > 0] > 0).all() and (got["TTSummedEnergy_se"][:, 0] <= E * (1 + 1e-12)).all()
    cq, cq_se, curve = got["TTPLCQ_Summed"][0], got["TTPLCQ_Summed_se"][0], got["TTNormCurve"][:, 0]
    print(f"lit rows: {lit.sum()} of {A}; lit by more than one batch: {lit_by_many}; fit c, q = {cq[0]:.4g}, {cq[1]:.4g} "
          f"+- (ln c) {cq_se[0]:.3g}, {cq_se[1]:.3g}")
    assert lit.sum() >= 1 and lit_by_many >= 1 and np.isfinite(cq_se).any()
    # normcurve_fitpowerlaw.m on the file's own numbers: polyfit of log E on log linspace(distances) over points 4 .. 48
    if (E[3:48] > 0).all():
        X = np.linspace(dist[0], dist[-1], A)
        P = np.polyfit(np.log(X[3:48]), np.log(E[3:48]), 1)
        assert cq[1] == pytest.approx(P[0], rel=1e-9) and cq[0] == pytest.approx(math.exp(P[1]), rel=1e-9)
        assert np.allclose(curve, cq[0] * X ** cq[1], rtol=1e-12)
        # arrayimage.m:54-59 from the curve and the traces
        for i in np.flatnonzero(lit)[:6]:
            row = read_octave(tt / f"seis_{48 + i:03d}.octv")["TraceXYZ"].sum(axis=1)
            assert np.allclose(got["TTImageCurve"][i], np.sqrt(row / (curve[i] / (n_bins * dt))), rtol=1e-5, atol=0)
        assert np.isfinite(got["TTImageCurve_se"]).all()
    else:
        assert np.isnan(cq).all() and np.isnan(curve).all() and np.isnan(got["TTImageCurve"]).all()
