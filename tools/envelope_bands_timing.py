"""What the bootstrap bands cost next to the envelope shape on the same blocks, and next to the batched run that made them:
one JSON line.

    python tools/envelope_bands_timing.py [out.json] [histories] [replicates]          (none, 10000000, 1000)

Crust-pinch model at TOA degree 9, B = 16 batches, the array all 480 receivers, every receiver's window from the default
phase edge to the end of the trace (Model.envshape_plan), SMOOTH 8, weights 1, 1, 1, R = 1000 replicates at the 90 % level.
Medians of 5 after a warm-up, with the spread.
(a) the run: Engine.run_batched_envelope_bands against Engine.run_batched of the same ids, wall clock: what the bands add to a
    run that has to be made anyway, per call and as a share of it.
(b) the kernels alone on the kept blocks of such a run, by device events around `inner` launches: r3d_envelope_bands with every
    output and with the six numbers only, r3d_envelope_shape with every output beside them, and r3d_bootstrap_counts_device;
    the bands stage as a share of the run that made the blocks.
No threshold is asserted anywhere."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radiative3d_amd import Engine, Model, _ffi, envelope_bands, envelope_shape  # noqa: E402
from radiative3d_amd.configs import CONFIGS  # noqa: E402
from radiative3d_amd.model import bands_tail  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
R = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
B, reps, inner, seed, smooth, level, bands_seed = 16, 5, 3, 0x5EED, 8, 0.9, 0xB007
T = bands_tail(R, level)
WEIGHTS = (1.0, 1.0, 1.0, 0.0, 0.0)
dev = torch.device("cuda", 0)
med = statistics.median


def spread(t):
    t = sorted(t)
    return {"ms": round(med(t), 4), "ms_min_max": [round(t[0], 4), round(t[-1], 4)]}


def wall(fn):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def timed(fn):
    fn()
    torch.cuda.synchronize()
    return [event_ms(fn) for _ in range(reps)]


model = Model(CONFIGS["crustpinch"](9))
S, n_bins = model.n_seismometers, model.n_bins
_, bins, _ = model.envshape_plan(dict(first=0, last=S - 1))
window_bins = int((bins[:, 1].astype(np.int64) - bins[:, 0]).sum())

# (a) the run
e = Engine(model)
plain = wall(lambda: e.run_batched(n, B, seed=seed))
banded = wall(lambda: e.run_batched_envelope_bands(n, B, bins, 0, S - 1, WEIGHTS, smooth, R, T, bands_seed, seed=seed))
added = med(banded) - med(plain)

# (b) the kernels alone, on the kept blocks of such a run
be = e.run_batched(n, B, seed=seed, keep_batches=True)[3]
e.close()
dbe = torch.from_numpy(be).to(dev)
dbins = torch.from_numpy(bins.view(np.int32)).to(dev)
L = _ffi.hip_lib()
dcounts = torch.empty(R * B, dtype=torch.uint8, device=dev)
stream = torch.cuda.current_stream(dev).cuda_stream
counts = timed(lambda: L.r3d_bootstrap_counts_device(0, bands_seed, B, R, dcounts.data_ptr(), stream))
everything = timed(lambda: envelope_bands(dbe, dbins, 0, S - 1, WEIGHTS, smooth, R, T, bands_seed))
numbers_only = timed(lambda: envelope_bands(dbe, dbins, 0, S - 1, WEIGHTS, smooth, R, T, bands_seed, with_envelope=False))
shape = timed(lambda: envelope_shape(dbe, dbins, 0, S - 1, WEIGHTS, smooth))

line = json.dumps({
    "config": "crustpinch", "toa_degree": 9, "histories": n, "batches": B, "receivers": S, "bins": n_bins, "smooth": smooth,
    "replicates": R, "tail": T, "weights": WEIGHTS, "reps": reps, "launches_per_sample": inner, "window_bins": window_bins,
    "run": {"run_batched": spread(plain), "run_batched_envelope_bands": spread(banded), "added_ms_per_call": round(added, 3),
            "added_share_of_run": round(added / med(plain), 5)},
    "kernel": {"bootstrap_counts": spread(counts), "bands_all_outputs": spread(everything),
               "bands_six_numbers_only": spread(numbers_only), "envelope_shape_all_outputs": spread(shape),
               "bands_over_shape": round(med(everything) / med(shape), 1),
               "bands_share_of_the_run_that_made_the_blocks": round(med(everything) / med(plain), 5)},
})
print(line, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
