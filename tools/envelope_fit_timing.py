"""What the envelope misfit costs on the device, next to the envelope shape on the same blocks: one JSON line.

    python tools/envelope_fit_timing.py [out.json] [histories]          (none, 10000000)

Crust-pinch model at TOA degree 9 (the benchmark's array shape), B = 16 batches, the array all 480 receivers, every
receiver's window from the default phase edge to the end of the trace (Model.envshape_plan), SMOOTH 8 over the synthetic and
1 over the observed row, weights 1, 1, 1, amplitudes.  The observed rows are the run's own envelope two bins later and half
as high.  On the kept blocks of ONE batched run, in ONE process, by device events around `inner` launches, medians of 5 after
a warm-up, with the spread, alternating the three:
    r3d_envelope_shape with every output             the sibling, the yardstick that is not the code under test
    r3d_envelope_misfit with every output, Lmax = 0   one lag: the rows, the passes and the sums
    r3d_envelope_misfit with every output, Lmax = 64  129 lags: the lag scan on top
and the ratios of the medians.  No threshold is asserted anywhere.

Measured on an MI355X, 1e7 histories (profiles/r06/envelope_fit_timing.json; LOG.md has the table): the shape 0.161 ms, the
misfit 0.173 ms with one lag (1.07 x the shape) and 0.474 ms with 129 lags (2.95 x the shape, 2.75 x one lag)."""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radiative3d_amd import Engine, Model, envelope_misfit, envelope_shape  # noqa: E402
from radiative3d_amd.configs import CONFIGS  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
B, reps, inner, seed, smooth, smooth_obs = 16, 5, 20, 0x5EED, 8, 1
WEIGHTS = (1.0, 1.0, 1.0, 0.0, 0.0)
dev = torch.device("cuda", 0)
med = statistics.median


def spread(t):
    t = sorted(t)
    return {"ms": round(med(t), 4), "ms_min_max": [round(t[0], 4), round(t[-1], 4)]}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


model = Model(CONFIGS["crustpinch"](9))
S, n_bins = model.n_seismometers, model.n_bins
assert S == 480
_, bins, _ = model.envshape_plan(dict(first=0, last=S - 1))
window_bins = int((bins[:, 1].astype(np.int64) - bins[:, 0]).sum())

e = Engine(model)
be = e.run_batched(n, B, seed=seed, keep_batches=True)[3]
e.close()
dbe = torch.from_numpy(be).to(dev)
dbins = torch.from_numpy(bins.view(np.int32)).to(dev)
own = envelope_misfit(dbe, dbins, torch.ones((S, n_bins), dtype=torch.float64, device=dev), 0, S - 1, WEIGHTS, smooth, 0, 0, 1)["envelope"]
obs = torch.zeros((S, n_bins), dtype=torch.float64, device=dev)
obs[:, 2:] = 0.5 * own[:, :-2]

calls = {
    "envelope_shape": lambda: envelope_shape(dbe, dbins, 0, S - 1, WEIGHTS, smooth),
    "envelope_misfit_lag_0": lambda: envelope_misfit(dbe, dbins, obs, 0, S - 1, WEIGHTS, smooth, smooth_obs, 0, 1),
    "envelope_misfit_lag_64": lambda: envelope_misfit(dbe, dbins, obs, 0, S - 1, WEIGHTS, smooth, smooth_obs, 64, 1),
}
for fn in calls.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {name: [] for name in calls}
for _ in range(reps):                       # alternating: what else the machine does falls on all three alike
    for name, fn in calls.items():
        times[name].append(event_ms(fn))
fit = calls["envelope_misfit_lag_64"]()
torch.cuda.synchronize()
lit = fit["lit"].cpu().numpy().astype(bool)
lag = fit["misfit"][:, 4].cpu().numpy()

shape_ms = med(times["envelope_shape"])
rows = B + 1
line = json.dumps({
    "config": "crustpinch", "toa_degree": 9, "histories": n, "batches": B, "receivers": S, "bins": n_bins, "smooth": smooth,
    "smooth_obs": smooth_obs, "weights": WEIGHTS, "reps": reps, "launches_per_sample": inner, "window_bins": window_bins,
    "row_sums_of_the_lag_scan": {"lag_0": S * rows, "lag_64": S * rows * 129},
    "products_of_the_lag_scan_lag_64": window_bins * rows * 129,
    "kernel": {name: spread(t) for name, t in times.items()},
    "over_envelope_shape": {name: round(med(t) / shape_ms, 3) for name, t in times.items() if name != "envelope_shape"},
    "lag_64_over_lag_0": round(med(times["envelope_misfit_lag_64"]) / med(times["envelope_misfit_lag_0"]), 3),
    "lit": int(lit.sum()), "lit_with_lag_2": int((lag[lit] == 2.0).sum()),
})
print(line, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
