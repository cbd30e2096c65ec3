"""The travel-time image above the kernel, without a GPU: the refusals of r3d_array_image (all made before any HIP call), the
--ttimage options of the command line, the array's plan, ttimage.octv, the structs' layouts and the add-on's place."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import radiative3d_amd
from cli_support import main_exe
from octave_text import read_octave
from radiative3d_amd import Model, _ffi
from radiative3d_amd.model import array_image_spec
from tests.configs import halfspace

REPO = _ffi.REPO
INCLUDE = os.path.join(REPO, "include")


# ---- refusals of the device call: all made before any HIP call, so they run here ------------------------------------
def test_array_image_refusals_come_before_any_device():
    L = _ffi.hip_lib()
    p = C.c_void_p(4096)                                           # (never dereferenced)

    def call(n_batches=2, blocks=p, image=p, se=p, null_spec=False, **kw):
        spec = array_image_spec(kw.pop("S", 5), kw.pop("n_bins", 40), kw.pop("first", 1), kw.pop("last", 3),
                                kw.pop("weights", (1, 1, 1, 0, 0)), kw.pop("k", 1), kw.pop("rho", 0.3), kw.pop("curve", None),
                                kw.pop("Tw", 0.0))
        for k, v in kw.items():
            setattr(spec, k, v)
        rc = L.r3d_array_image(0, n_batches, blocks, None if null_spec else C.byref(spec), image, se, p, p, p, p, p, None)
        return rc, L.r3d_last_error().decode()

    for kw, why in ((dict(n_batches=0), "n_batches == 0"), (dict(n_batches=65), "at most 64"), (dict(blocks=None), "null"),
                    (dict(image=None), "null"), (dict(null_spec=True), "null array spec"), (dict(size=8), "size"),
                    (dict(n_bins=0), "n_bins"), (dict(first=3, last=2), "not within"), (dict(last=5), "not within"),
                    (dict(weights=(1, -0.5, 1, 0, 0)), "weight 1 is negative or not finite"),
                    (dict(weights=(1, 1, 1, 0, math.inf)), "weight 4 is negative or not finite"),
                    (dict(weights=(math.nan, 1, 1, 0, 0)), "weight 0"), (dict(k=3), "gamma_log2"),
                    (dict(rho=-0.01), "rho"), (dict(rho=1.01), "rho"), (dict(rho=math.nan), "rho"), (dict(mode=7), "mode"),
                    (dict(mode=_ffi.R3D_ARRAY_CURVE, Tw=20.0), "without curve values"),
                    (dict(curve=4096, Tw=0.0), "window_length"), (dict(curve=4096, Tw=math.inf), "window_length"),
                    (dict(curve=4096, Tw=math.nan), "window_length"), (dict(n_batches=1), "at least 2 batches")):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("r3d_array_image: ") and why in msg, (kw, msg)
    import torch
    if not torch.cuda.is_available():
        # a well-formed call gets as far as the device, and no further
        for kw in (dict(), dict(n_batches=1, se=None), dict(curve=4096, Tw=20.0)):
            rc, msg = call(**kw)
            assert rc != 0 and msg == "r3d_array_image: no HIP device (or a bad device index)"


def test_run_batched_array_image_refuses_before_the_engine_is_looked_at(models):
    L = _ffi.hip_lib()
    m = models("halfspace", 3)
    res = m.new_result()
    c = res._as_c()
    spec = array_image_spec(m.n_seismometers, m.n_bins, 0, 9, (1, 1, 1, 0, 0))
    image = np.full((10, m.n_bins), -2.0)
    out = _ffi.ArrayImageResult(size=C.sizeof(_ffi.ArrayImageResult), image=image.ctypes.data)
    assert L.r3d_run_batched_array_image(None, 1000, 0, 1, 4, C.byref(c), None, None, C.byref(spec), C.byref(out)) != 0
    assert "null engine" in L.r3d_last_error().decode() and (image == -2.0).all() and not res.energy.any()


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_ttimage_options_parse_and_are_off_by_default():
    assert Model(halfspace(3)).ttimage_request is None
    rq = Model(halfspace(3) + ["--error-batches=8", "--ttimage"]).ttimage_request
    assert all(math.isnan(v) for v in rq["curve"])
    assert dict(rq, curve=None) == dict(first=0, last=143, gamma_log2=1, norm=0.3, axes=(1.0, 1.0, 1.0), fit=(0, 0), curve=None)
    m = Model(halfspace(3) + ["--error-batches=8", "--ttimage=4,0.5", "--ttimage-array=48,95", "--ttimage-axes=0,0,1",
                              "--ttimage-fit=4,48", "--ttimage-normcurve=2.5e-3,-1.75"])
    assert m.ttimage_request == dict(first=48, last=95, gamma_log2=2, norm=0.5, axes=(0.0, 0.0, 1.0), fit=(4, 48),
                                     curve=(2.5e-3, -1.75))
    assert Model(halfspace(3) + ["--error-batches=8", "--ttimage=1,0"]).ttimage_request["gamma_log2"] == 0
    with pytest.raises(RuntimeError, match="0 .. 143"):
        Model(halfspace(3) + ["--error-batches=8", "--ttimage", "--ttimage-array=48,144"]).ttimage_request
    with pytest.raises(RuntimeError, match="points 1 .. 48"):
        Model(halfspace(3) + ["--error-batches=8", "--ttimage", "--ttimage-array=48,95", "--ttimage-fit=4,49"]).ttimage_request


REFUSED = [(["--ttimage-array=0,47"], "--ttimage-array needs --ttimage"),
           (["--ttimage-axes=1,1,1"], "--ttimage-axes needs --ttimage"),
           (["--ttimage-fit=4,48"], "--ttimage-fit needs --ttimage"),
           (["--ttimage-normcurve=1,-2"], "--ttimage-normcurve needs --ttimage"),
           (["--ttimage"], "--ttimage needs --error-batches"),
           (["--ttimage", "--job-error-batches=4"], "ONE device's"),
           (["--ttimage", "--error-batches=8", "--lapse-windows"], "out of scope"),
           (["--ttimage", "--error-batches=8", "--ttimage-normcurve=1,-2"], "range window comes from the fit's array"),
           (["--ttimage=3,0.3", "--error-batches=8"], "GAMMA must be 1, 2 or 4"),
           (["--ttimage=2,1.5", "--error-batches=8"], "must lie in [0, 1]"),
           (["--ttimage=2", "--error-batches=8"], "Required value not provided"),
           (["--ttimage", "--error-batches=8", "--ttimage-array=5,2"], "FIRST <= LAST"),
           (["--ttimage", "--error-batches=8", "--ttimage-axes=1,-1,1"], "not negative"),
           (["--ttimage", "--error-batches=8", "--ttimage-fit=5,5"], "IBEGIN < IEND"),
           (["--ttimage", "--error-batches=8", "--ttimage-fit=4,48", "--ttimage-normcurve=0,-2"], "C > 0")]


@pytest.mark.parametrize("extra,message", REFUSED)
def test_cli_refuses_ttimage_options_at_parse_time(tmp_path, extra, message):
    with pytest.raises(RuntimeError, match=re.escape(message)):
        Model(halfspace(3) + extra)
    r = subprocess.run([main_exe()] + halfspace(3) + ["--num-phonons=1K", f"--output-dir={tmp_path}"] + extra, cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Error processing command-line options" in r.stdout and message in r.stdout, r.stdout[-2000:]
    assert not list(tmp_path.iterdir())                            # nothing written, no device looked for


def test_help_names_the_ttimage_options_and_what_is_out_of_scope():
    text = subprocess.run([main_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    for name in ("--ttimage[=GAMMA,NORM]", "--ttimage-array", "--ttimage-axes", "--ttimage-fit", "--ttimage-normcurve",
                 "Not in one run with --lapse-windows"):
        assert name in text


# ---- the plan and ttimage.octv ------------------------------------------------------------------------------------------------
def test_the_plan_is_range_km_and_azimuth_deg_and_shares_the_lapse_plans_distances():
    m = Model(halfspace(3) + ["--error-batches=8", "--ttimage", "--ttimage-array=48,95"])
    dist, azi = m.ttimage_plan()
    lapse = dict(first=48, last=95, phase_edge=(3.6, 0.0), windows=(5.0, 20.0, 45.0, 115.0), axes=(0, 0, 1), geospread=2.0,
                 ranges=(8.0, 50.0, 150.0))
    assert (dist == m.lapse_plan(lapse)[0]).all() and (dist > 0).all()
    assert ((azi >= 0) & (azi < 360)).all()
    assert len(m.ttimage_plan(dict(first=0, last=143))[0]) == 144
    with pytest.raises(RuntimeError, match="not within"):
        m.ttimage_plan(dict(first=0, last=144))


def test_write_ttimage_round_trips_every_value_at_17_digits(tmp_path):
    m = Model(halfspace(3) + ["--error-batches=8", "--ttimage=4,0.25", "--ttimage-array=48,95", "--ttimage-fit=4,48"])
    plan = m.ttimage_plan()
    A, n_bins, B, dt = 48, m.n_bins, 8, 0.5
    rng = np.random.default_rng(22)
    img = dict(image=rng.random((A, n_bins)), image_se=rng.random((A, n_bins)) * 0.1, lit=rng.integers(0, 2, A).astype(np.uint32),
               summed=rng.lognormal(0, 1, A), summed_se=rng.lognormal(-2, 1, A), peak=rng.lognormal(0, 1, A),
               peak_bin=rng.integers(0, n_bins, A).astype(np.uint32))
    path = tmp_path / "ttimage.octv"
    m.write_ttimage(path, plan, img, B)
    got = read_octave(path)
    assert len(got) == 16 and "TTFitRange" not in got               # an image without a fit's results: no fit items
    with_fit = dict(img, fit=(812.5, -1.625), fit_se=(0.25, math.nan), curve_made=True, curve=rng.lognormal(0, 1, A),
                    image_curve=rng.random((A, n_bins)), image_curve_se=rng.random((A, n_bins)))
    with_fit["image_curve_se"][3, 7] = math.nan
    m.write_ttimage(path, plan, with_fit, B)
    got = read_octave(path)
    assert len(got) == 22
    assert (got["TTSeismometers"][:, 0] == np.arange(48, 96)).all() and got["TTBatches"] == B and got["TTNumBins"] == n_bins
    assert (got["TTDistances"][:, 0] == plan[0]).all() and (got["TTAzimuths"][:, 0] == plan[1]).all()
    assert got["TTTimeWindow"].tolist() == [[0.0, n_bins * dt]] and got["TTAxes"].tolist() == [[1.0, 1.0, 1.0]]
    assert got["TTGamma"] == 4 and got["TTNorm"] == 0.25
    assert (got["TTImage"] == img["image"]).all() and (got["TTImage_se"] == img["image_se"]).all()
    assert (got["TTLit"][:, 0] == img["lit"]).all() and (got["TTPeakBin"][:, 0] == img["peak_bin"]).all()
    assert (got["TTSummedEnergy"][:, 0] == img["summed"] * dt).all() and (got["TTSummedEnergy_se"][:, 0] == img["summed_se"] * dt).all()
    assert (got["TTPeakEnergy"][:, 0] == img["peak"]).all()
    assert got["TTFitRange"].tolist() == [[4, 48]] and got["TTPLCQ_Summed"].tolist() == [[812.5, -1.625]]
    assert got["TTPLCQ_Summed_se"][0, 0] == 0.25 and math.isnan(got["TTPLCQ_Summed_se"][0, 1])
    assert (got["TTNormCurve"][:, 0] == with_fit["curve"]).all() and (got["TTImageCurve"] == with_fit["image_curve"]).all()
    se = got["TTImageCurve_se"]
    assert math.isnan(se[3, 7]) and (np.nan_to_num(se, nan=-1.0) == np.nan_to_num(with_fit["image_curve_se"], nan=-1.0)).all()
    with pytest.raises(RuntimeError, match="at least 2 batches"):
        m.write_ttimage(path, plan, img, 1)


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------
def test_new_structs_mirror_the_c_layout(tmp_path):
    pairs = (("r3d_array_image_spec", _ffi.ArrayImageSpec), ("r3d_array_image_result", _ffi.ArrayImageResult),
             ("r3dh_ttimage_opts", _ffi.TTImageOpts), ("r3dh_ttimage_result", _ffi.TTImageResult))
    lines = []
    for name, mirror in pairs:
        lines.append(f'printf("%zu\\n", sizeof({name}));')
        lines += [f'printf("%zu\\n", offsetof({name}, {field[0]}));' for field in mirror._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "r3d_host.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n"
    src = tmp_path / "s.c"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(tmp_path / "s"), str(src)])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    want = []
    for name, mirror in pairs:
        want += [C.sizeof(mirror)] + [getattr(mirror, field[0]).offset for field in mirror._fields_]
    assert got == want


def test_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(INCLUDE, "r3d.h")).read()
    L, H = _ffi.hip_lib(), _ffi.host_lib()
    for name, n_args in (("r3d_array_image", 12), ("r3d_array_powerlaw", 8), ("r3d_array_powerlaw_jackknife", 11),
                         ("r3d_run_batched_array_image", 10)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        f = getattr(L, name)
        assert len(f.argtypes) == n_args and f.restype is C.c_int, name
        assert getattr(_ffi.hip_lib(reproducible=True), name)
    assert "r3d_node_run_batched) has no image call" in header and "cannot be combined with r3d_run_batched_windows" in header
    host_header = open(os.path.join(INCLUDE, "r3d_host.h")).read()
    for name in ("r3dh_ttimage_request", "r3dh_ttimage_plan", "r3dh_write_ttimage"):
        assert name in host_header and getattr(H, name).argtypes
    for name in ("array_image", "array_powerlaw"):
        assert callable(getattr(radiative3d_amd, name))
    assert callable(radiative3d_amd.Engine.run_batched_array_image) and callable(Model.ttimage_plan)


def test_the_array_image_lives_in_an_add_on_of_its_own():
    """One .hip and one header, on include/r3d.h and common/r3d_entry.h, nothing from csrc/ and nothing of it in the hashed
    kernel sources; no update of memory shared between workgroups; the window header is a prerequisite in the Makefile."""
    arrays = os.path.join(REPO, "radiative3d_amd", "arrays")
    assert sorted(os.listdir(arrays)) == ["r3d_array_image.h", "r3d_array_image.hip"]
    csrc = os.path.join(REPO, "radiative3d_amd", "csrc")
    for f in os.listdir(csrc):
        assert "array_image" not in open(os.path.join(csrc, f), errors="ignore").read(), f
    text = re.sub(r"//[^\n]*", "", open(os.path.join(arrays, "r3d_array_image.hip")).read())
    assert "csrc/" not in text and "atomic" not in text and '#include "../common/r3d_entry.h"' in text
    head = open(os.path.join(arrays, "r3d_array_image.h")).read()
    assert '#include "../stats/r3d_window_sums.h"' in head and "pow(" not in re.sub(r"//[^\n]*", "", head)
    make = open(os.path.join(REPO, "Makefile")).read()
    assert re.search(r"^ADDONS := .*\barrays\b", make, re.M) and "$(filter arrays,$(1)),radiative3d_amd/stats/r3d_window_sums.h" in make
