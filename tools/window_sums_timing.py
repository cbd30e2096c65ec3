"""What the lapse-window sums cost, and how well their standard errors are calibrated: one JSON line.

    python tools/window_sums_timing.py [out.json] [histories]          (none, 10000000)

(i)   r3d_window_sums (energies and counts) over B = 64 batch blocks of NSCP's shape, 480 seismometers x 300 bins, on three
      window shapes -- the lapse shape (lapsetimecurve.m's two windows per receiver, the crust-pinch run's own distances),
      decimation by 4 (75 windows of 4 bins: vis/seisplot/decimate.m) and one whole-trace window per receiver -- each
      against a device-to-device copy of the BYTES THOSE WINDOWS COVER (energy 40 + counts 16 per bin and batch), the
      yardstick that is not the code under test, timed in the same process with events on the stream.  Every sample is
      `inner` launches between two events; medians of 5 samples after a warm-up, with the spread.
(ii)  calibration: two batched half-space runs of disjoint id ranges with the lapse windows summed on the device
      (r3d_run_batched_windows), z = (T1 - T2) / sqrt(se1^2 + se2^2) over the windows with at least 25 catches in both
      runs; its r.m.s. is 1 for an honest standard error."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radiative3d_amd import Engine, Model, batch_moments, window_sums  # noqa: E402
from radiative3d_amd.configs import CONFIGS  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
B, reps, inner, seed = 64, 5, 20, 0x5EED
LAPSE = dict(phase_edge=(3.6, 0.0), windows=(5.0, 20.0, 45.0, 115.0), axes=(0.0, 0.0, 1.0), geospread=2.0,
             ranges=(8.0, 50.0, 150.0))
WEIGHTS = LAPSE["axes"] + (0.0, 0.0)
dev = torch.device("cuda", 0)

# ---- (i) the kernel against a copy ------------------------------------------------------------------------------------
nscp = Model(CONFIGS["crustpinch"](4))
S, n_bins = nscp.n_seismometers, nscp.n_bins
assert (S, n_bins) == (480, 300)
_, lapse_bins, _ = nscp.lapse_plan(dict(LAPSE, first=0, last=S - 1))
edges = np.arange(0, n_bins + 1, 4, dtype=np.uint32)
shapes = {
    "lapse": lapse_bins,
    "decimate_4": np.broadcast_to(np.stack([edges[:-1], edges[1:]], axis=1), (S, len(edges) - 1, 2)).copy(),
    "whole_trace": np.broadcast_to(np.array([[0, n_bins]], dtype=np.uint32), (S, 1, 2)).copy(),
}
gen = torch.Generator(device=dev).manual_seed(seed)
be = torch.rand((B, S, n_bins, 5), dtype=torch.float64, device=dev, generator=gen)
bc = torch.randint(0, 50, (B, S, n_bins, 2), dtype=torch.int64, device=dev, generator=gen)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return sorted(event_ms(fn) for _ in range(reps))


results = {}
for shape, bins in shapes.items():
    dbins = torch.from_numpy(bins.view(np.int32)).to(dev)
    W = bins.shape[1]
    y = torch.empty((B, S, W), dtype=torch.float64, device=dev)
    yc = torch.empty((B, S, W, 2), dtype=torch.int64, device=dev)
    covered = int((bins[..., 1].astype(np.int64) - bins[..., 0]).sum()) * B * (40 + 16)
    src = torch.empty(covered // 8, dtype=torch.int64, device=dev).random_(generator=gen)
    dst = torch.empty_like(src)
    k = timed(lambda: window_sums(be, dbins, WEIGHTS, batch_counts=bc, window_energy=y, window_counts=yc))
    c = timed(lambda: dst.copy_(src, non_blocking=True))
    total, totalc, _, se, _ = batch_moments(y, yc)
    m = timed(lambda: batch_moments(y, yc, energy=total, counts=totalc))
    med = statistics.median
    results[shape] = {
        "windows_per_seismometer": W, "bytes_covered": covered, "bytes_written": y.numel() * 8 + yc.numel() * 8,
        "kernel_ms": round(med(k), 5), "kernel_ms_min_max": [round(k[0], 5), round(k[-1], 5)],
        "kernel_GBps": round(covered / med(k) / 1e6, 1),
        "copy_ms": round(med(c), 5), "copy_ms_min_max": [round(c[0], 5), round(c[-1], 5)],
        "copy_GBps_read": round(covered / med(c) / 1e6, 1),
        "kernel_over_copy": round(med(k) / med(c), 3),
        "moments_of_the_sums_ms": round(med(m), 5),
    }
    del src, dst
del be, bc
torch.cuda.empty_cache()

# ---- (ii) calibration on two disjoint id ranges of the half-space run -----------------------------------------------------
half = Model(CONFIGS["halfspace"](4))
e = Engine(half)
_, hbins, _ = half.lapse_plan(dict(LAPSE, first=0, last=half.n_seismometers - 1))
r1 = e.run_batched_windows(n, B, hbins, WEIGHTS, first_id=0, seed=seed)
r2 = e.run_batched_windows(n, B, hbins, WEIGHTS, first_id=n, seed=seed)
t1, c1, s1 = r1[3], r1[4].sum(-1), r1[5]
t2, c2, s2 = r2[3], r2[4].sum(-1), r2[5]
both = (c1 >= 25) & (c2 >= 25)
z = (t1[both] - t2[both]) / np.sqrt(s1[both] ** 2 + s2[both] ** 2)
e.close()

line = json.dumps({
    "shape": {"seismometers": S, "bins": n_bins, "batches": B}, "reps": reps, "launches_per_sample": inner,
    "weights": WEIGHTS, "cases": results,
    "calibration": {"config": "halfspace", "toa_degree": 4, "histories_per_run": n, "batches": B,
                    "windows_with_25_catches_in_both": int(both.sum()), "windows": int(both.size),
                    "z_rms": round(float(np.sqrt(np.mean(z ** 2))), 4) if both.any() else None},
})
print(line, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
