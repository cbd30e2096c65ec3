"""What the slant stack costs on the device, stage by stage, next to two yardsticks: one JSON line.

    make -j16 variant NAME=SLANT
    python tools/slant_stack_timing.py [out.json] [histories]          (none, 10000000)

Crust-pinch model at TOA degree 9 (the NSCP workload's array shape: 160 receivers of 300 bins), B = 16 batches, the array the
model's first line of 160 receivers, M = 64 slownesses 0 .. 0.35 s/km about the middle of the line, SMOOTH 2, amplitudes, the
gains (r / r_ref)^0.5, two windows.  On the kept blocks of ONE batched run, in ONE process.  The stages' device times come from
a developer build of the library (R3D_HIP_LIB, default radiative3d_amd/lib/variant_SLANT.so), whose r3d_slant_stack_stages
records device events around the launches of r3d_slant_stack: the rows | the stack | everything behind it (the se of the
stack, the curves, the picks, the counts).  Medians of 7 calls after a warm-up, with the spread, for the call with every se
(17 rows) and for the call without (1 row).  Beside them, by device events of the same kind:
    the batched run the stack follows (Engine.run_batched of the same histories, kept blocks: wall clock, it includes the host)
    reading the row scratch once: a sum over rows x A x n_bins doubles -- what the stack kernel would take if every row value
    came in once and nothing else cost anything
No threshold is asserted anywhere: nobody had measured this kernel.

Measured on an MI355X, 1e7 histories (profiles/r06/slant_stack_timing.json; LOG.md has the table): with every se rows 0.058 ms,
stack 0.783 ms, the rest 0.074 ms; without an se 0.034, 0.077 and 0.059 ms; reading the row scratch once 0.016 and 0.010 ms; the
batched run 61 ms."""
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

from radiative3d_amd import Engine, Model, _ffi, slant_shifts  # noqa: E402
from radiative3d_amd.configs import CONFIGS  # noqa: E402
from radiative3d_amd.model import slant_spec  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
B, reps, seed, smooth, M, first, last = 16, 7, 0x5EED, 2, 64, 0, 159
WEIGHTS = (1.0, 1.0, 1.0, 0.0, 0.0)
dev = torch.device("cuda", 0)
med = statistics.median


def spread(t):
    t = sorted(t)
    return {"ms": round(med(t), 4), "ms_min_max": [round(t[0], 4), round(t[-1], 4)]}


model = Model(CONFIGS["crustpinch"](9) + ["--error-batches=16", "--slant-stack=0,0.35,64,nan,2", "--slant-array=0,159",
                                         "--slant-range-power=0.5", "--slant-windows=0,600,100,300"])
plan = model.slant_plan()
S, n_bins, A = model.n_seismometers, model.n_bins, last - first + 1
assert S == 480 and plan["shift_bin"].shape == (M, A)

e = Engine(model)
e.run_batched(n // 10, B, seed=seed)
t0 = time.perf_counter()
be = e.run_batched(n, B, seed=seed, keep_batches=True)[3]
run_ms = (time.perf_counter() - t0) * 1e3
e.close()
dbe = torch.from_numpy(be).to(dev)
k, f = torch.from_numpy(plan["shift_bin"]).to(dev), torch.from_numpy(plan["shift_frac"]).to(dev)
g, win = torch.from_numpy(plan["gain"]).to(dev), torch.from_numpy(plan["windows"].view(np.int32)).to(dev)
W = win.shape[0]
spec = slant_spec(S, n_bins, first, last, WEIGHTS, k.data_ptr(), f.data_ptr(), g.data_ptr(), win.data_ptr(), M, W, plan["p0"], plan["dp"],
                  smooth, 1)
lib = C.CDLL(os.environ.get("R3D_HIP_LIB") or os.path.join(_ffi.LIBDIR, "variant_SLANT.so"))
lib.r3d_slant_stack_stages.restype = C.c_int
lib.r3d_slant_stack_stages.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.POINTER(_ffi.SlantSpec)] + [C.c_void_p] * 10 + [C.POINTER(C.c_float)]
lib.r3d_last_error.restype = C.c_char_p
out = {name: torch.empty(shape, dtype=torch.float64, device=dev) for name, shape in
       (("stack", (M, n_bins)), ("stack_se", (M, n_bins)), ("power", (W, M)), ("power_se", (W, M)), ("picks", (W, 4)), ("picks_se", (W, 4)))}
fold = torch.empty((M, n_bins), dtype=torch.int32, device=dev)
counts = torch.zeros(2, dtype=torch.int64, device=dev)


def stages(with_se):
    ms = (C.c_float * 3)()
    se = lambda name: out[name].data_ptr() if with_se else None   # noqa: E731
    rc = lib.r3d_slant_stack_stages(0, B, dbe.data_ptr(), C.byref(spec), out["stack"].data_ptr(), se("stack_se"), fold.data_ptr(),
                                    out["power"].data_ptr(), se("power_se"), out["picks"].data_ptr(), se("picks_se"),
                                    counts[0:].data_ptr(), counts[1:].data_ptr(), torch.cuda.current_stream(dev).cuda_stream, ms)
    assert rc == 0, lib.r3d_last_error().decode()
    return list(ms)


def read_once_ms(rows):
    v = torch.ones((rows, A, n_bins), dtype=torch.float64, device=dev)
    for _ in range(3):
        v.sum()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        v.sum()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return spread(t)


result = {}
for name, with_se in (("with_se", True), ("without_se", False)):
    for _ in range(3):
        stages(with_se)
    t = [stages(with_se) for _ in range(reps)]
    rows = B + 1 if with_se else 1
    result[name] = {"rows": rows, "rows_kernel": spread([x[0] for x in t]), "stack_kernel": spread([x[1] for x in t]),
                    "finish_kernels": spread([x[2] for x in t]), "read_the_row_scratch_once": read_once_ms(rows),
                    "samples_of_the_stack": rows * M * n_bins * A}
picks = out["picks"].cpu().numpy()
line = json.dumps({
    "config": "crustpinch", "toa_degree": 9, "histories": n, "batches": B, "receivers": A, "bins": n_bins, "slownesses": M,
    "windows": W, "smooth": smooth, "weights": WEIGHTS, "reps": reps, "batched_run_wall_ms": round(run_ms, 2),
    "stages": result, "picked_slowness": [round(float(v), 4) for v in picks[:, 1]], "bad_shifts": int(counts[1]),
})
print(line, flush=True)
if out_path:
    with open(out_path, "w") as f_:
        f_.write(line + "\n")
