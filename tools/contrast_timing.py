"""What the contrast of two runs costs on the device, stage by stage, next to two yardsticks: one JSON line.

    make -j16 variant NAME=CONTRAST
    python tools/contrast_timing.py [out.json] [histories a side]          (none, 10000000)

Crust-pinch model at TOA degree 9 (the NSCP workload's array shape: 160 receivers of 300 bins) as the base and the same model
without the pinch (PinchFrac 1) as the test, Ba = Bb = 16 batches, the array the model's first line of 160 receivers, SMOOTH 8,
three group-velocity windows, two regions, the gains (r / r_ref)^0.5.  On the kept blocks of TWO batched runs, in ONE process.
The stages' device times come from a developer build of the library (R3D_HIP_LIB, default radiative3d_amd/lib/variant_CONTRAST.so),
whose r3d_array_contrast_stages records device events around the launches of r3d_array_contrast: the rows kernel (rows, scale,
window sums, passes, pixels, windows: everything per receiver) | everything behind it (the regions, the counts).  Medians of 7
calls after a warm-up, with the spread, for the call with every se (17 rows a side) and for the call without (1 row a side).
Beside them:
    the two batched runs the contrast follows (Engine.run_batched of the same histories, kept blocks: wall clock, it includes
    the host)
    reading both block sets once by device events of the same kind: a sum over (Ba + Bb) x A x n_bins x 5 doubles -- what the
    rows kernel would take if every block value came in once and nothing else cost anything.  THE number to judge against.
No threshold is asserted anywhere: nobody had measured this kernel."""
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radiative3d_amd import Engine, Model, _ffi  # noqa: E402
from radiative3d_amd.configs import CONFIGS  # noqa: E402
from radiative3d_amd.model import contrast_spec  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
B, reps, seed, smooth, first, last = 16, 7, 0x5EED, 8, 0, 159
WEIGHTS = (1.0, 1.0, 1.0, 0.0, 0.0)
dev = torch.device("cuda", 0)
med = statistics.median


def spread(t):
    t = sorted(t)
    return {"ms": round(med(t), 4), "ms_min_max": [round(t[0], 4), round(t[-1], 4)]}


base_args = CONFIGS["crustpinch"](9)
model_args = [a for a in base_args if a.startswith("--model-args=")][0].split("=", 1)[1].split(",")
assert model_args[-4] == ".3666667"
flat = ",".join(model_args[:-4] + ["1.0"] + model_args[-3:])
model = Model(base_args + [f"--num-phonons={n}", "--error-batches=16", f"--array-contrast={smooth}", "--contrast-model-args=" + flat,
                           "--contrast-array=0,159", "--contrast-windows=8.0,4.6,4.6,3.7,3.7,3.0", "--contrast-regions=100,400,500,950",
                           "--contrast-range-power=0.5"])
plan = model.contrast_plan()
test_model = Model([a for a in base_args if not a.startswith("--model-args=")] + ["--model-args=" + flat])
S, n_bins, A = model.n_seismometers, model.n_bins, last - first + 1
W, R = plan["bins"].shape[1], plan["regions"].shape[0]
assert S == 480 and (W, R) == (3, 2) and test_model.n_bins == n_bins

blocks, run_ms = [], []
for m, s in ((model, seed), (test_model, seed + 1)):
    e = Engine(m)
    e.run_batched(n // 10, B, seed=s)
    t0 = time.perf_counter()
    blocks.append(torch.from_numpy(e.run_batched(n, B, seed=s, keep_batches=True)[3]).to(dev))
    run_ms.append((time.perf_counter() - t0) * 1e3)
    e.close()
xa, xb = blocks
bins, gain = torch.from_numpy(plan["bins"].view(np.int32)).to(dev), torch.from_numpy(plan["gain"]).to(dev)
spec = contrast_spec(S, n_bins, first, last, WEIGHTS, bins.data_ptr(), gain.data_ptr(), W, [tuple(v) for v in plan["regions"]], (1.0, 1.0), smooth)
lib = C.CDLL(os.environ.get("R3D_HIP_LIB") or os.path.join(_ffi.LIBDIR, "variant_CONTRAST.so"))
lib.r3d_array_contrast_stages.restype = C.c_int
lib.r3d_array_contrast_stages.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(_ffi.ContrastSpec)] + \
    [C.c_void_p] * 10 + [C.POINTER(C.c_float)]
lib.r3d_last_error.restype = C.c_char_p
out = {name: torch.empty(shape, dtype=torch.float64, device=dev) for name, shape in
       (("contrast", (A, n_bins)), ("contrast_se", (A, n_bins)), ("window", (A, W, 3)), ("window_se", (A, W, 3)), ("region", (R, W, 3)),
        ("region_se", (R, W, 3)), ("region_loo", (R, W, 2 * B)))}
lit = torch.empty(A, dtype=torch.int32, device=dev)
bad = torch.zeros(1, dtype=torch.int64, device=dev)


def stages(with_se):
    ms = (C.c_float * 2)()
    se = lambda name: out[name].data_ptr() if with_se else None   # noqa: E731
    rc = lib.r3d_array_contrast_stages(0, B, xa.data_ptr(), B, xb.data_ptr(), C.byref(spec), out["contrast"].data_ptr(), se("contrast_se"),
                                       lit.data_ptr(), out["window"].data_ptr(), se("window_se"), out["region"].data_ptr(),
                                       se("region_se"), se("region_loo"), bad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream, ms)
    assert rc == 0, lib.r3d_last_error().decode()
    return list(ms)


def read_once_ms():
    """Both block sets' array rows, every double once (the sum reads what the rows kernel reads: 2 x 16 x 160 x 300 x 5 doubles)."""
    va, vb = xa[:, first:last + 1].contiguous(), xb[:, first:last + 1].contiguous()
    for _ in range(3):
        va.sum(), vb.sum()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        va.sum(), vb.sum()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return spread(t)


result = {}
for name, with_se in (("with_se", True), ("without_se", False)):
    for _ in range(3):
        stages(with_se)
    t = [stages(with_se) for _ in range(reps)]
    result[name] = {"rows_a_side": B + 1 if with_se else 1, "rows_kernel": spread([x[0] for x in t]),
                    "regions_and_counts": spread([x[1] for x in t])}
region = out["region"].cpu().numpy()
line = json.dumps({
    "config": "crustpinch against the same without the pinch", "toa_degree": 9, "histories_a_side": n, "batches_a_side": B, "receivers": A,
    "bins": n_bins, "windows": W, "regions": R, "smooth": smooth, "weights": WEIGHTS, "reps": reps,
    "batched_runs_wall_ms": [round(v, 2) for v in run_ms], "read_both_block_sets_once": read_once_ms(),
    "block_doubles_read": 2 * B * A * n_bins * 5, "stages": result,
    "region_ratio": [[round(float(v), 4) for v in row] for row in region[..., 2]], "lit": int(lit.sum()), "bad": int(bad[0]),
})
print(line, flush=True)
if out_path:
    with open(out_path, "w") as f_:
        f_.write(line + "\n")
