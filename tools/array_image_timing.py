"""What the array's travel-time image costs next to the batched run it follows: one JSON line.

    python tools/array_image_timing.py [out.json] [histories]          (none, 10000000)

(i)   r3d_array_image over B = 64 batch blocks of NSCP's shape, 480 receivers x 300 bins (every receiver in the array, gamma
      2, weights 1, 1, 1): the LEGACY image with its jackknife errors, the same without them (no leave-one-out rows), and the
      CURVE image with errors -- each against a device-to-device copy of the blocks' bytes (40 per bin and batch), the
      yardstick that is not the code under test, timed in the same process with events on the stream.  Every sample is
      `inner` launches between two events; medians of 5 samples after a warm-up, with the spread.
(ii)  the run: Engine.run_batched against Engine.run_batched_array_image (image, fit and curve image) on the crust-pinch
      model, wall clock, medians of 3 after a warm-up: what the image adds to a run that has to be made anyway.
No threshold is asserted anywhere."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from radiative3d_amd import Engine, Model, array_image  # noqa: E402
from radiative3d_amd.configs import CONFIGS  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
B, reps, inner, seed = 64, 5, 20, 0x5EED
WEIGHTS = (1.0, 1.0, 1.0, 0.0, 0.0)
dev = torch.device("cuda", 0)
med = statistics.median

nscp = Model(CONFIGS["crustpinch"](4))
S, n_bins = nscp.n_seismometers, nscp.n_bins
assert (S, n_bins) == (480, 300)
gen = torch.Generator(device=dev).manual_seed(seed)
be = torch.rand((B, S, n_bins, 5), dtype=torch.float64, device=dev, generator=gen)
curve = torch.rand(S, dtype=torch.float64, device=dev, generator=gen) + 0.5
image, image_se = torch.empty((S, n_bins), dtype=torch.float64, device=dev), torch.empty((S, n_bins), dtype=torch.float64, device=dev)
src = torch.empty(be.numel(), dtype=torch.int64, device=dev).random_(generator=gen)
dst = torch.empty_like(src)


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


def entry(t, copy):
    return {"ms": round(med(t), 5), "ms_min_max": [round(t[0], 5), round(t[-1], 5)], "over_copy": round(med(t) / med(copy), 3)}


c = timed(lambda: dst.copy_(src, non_blocking=True))
cases = {
    "legacy_with_se": timed(lambda: array_image(be, 0, S - 1, WEIGHTS, 1, 0.3, image=image, image_se=image_se)),
    "legacy_without_se": timed(lambda: array_image(be, 0, S - 1, WEIGHTS, 1, 0.3, with_se=False, image=image)),
    "curve_with_se": timed(lambda: array_image(be, 0, S - 1, WEIGHTS, 1, curve=curve, window_length=n_bins * 0.5, image=image,
                                               image_se=image_se)),
}
kernel = {name: entry(t, c) for name, t in cases.items()}
del be, src, dst
torch.cuda.empty_cache()

e = Engine(nscp)
dist, _ = nscp.ttimage_plan(dict(first=0, last=S - 1))


def wall(fn):
    fn()
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)


plain = wall(lambda: e.run_batched(n, B, seed=seed))
imaged = wall(lambda: e.run_batched_array_image(n, B, 0, S - 1, WEIGHTS, 1, 0.3, fit=(48, S), ranges=(dist[0], dist[-1]), seed=seed))
e.close()

line = json.dumps({
    "shape": {"receivers": S, "bins": n_bins, "batches": B}, "reps": reps, "launches_per_sample": inner, "weights": WEIGHTS,
    "blocks_bytes": B * S * n_bins * 40, "copy_ms": round(med(c), 5), "copy_ms_min_max": [round(c[0], 5), round(c[-1], 5)],
    "kernel": kernel,
    "run": {"config": "crustpinch", "toa_degree": 4, "histories": n, "batches": B,
            "run_batched_ms": round(med(plain), 3), "run_batched_ms_min_max": [round(plain[0], 3), round(plain[-1], 3)],
            "run_batched_array_image_ms": round(med(imaged), 3),
            "run_batched_array_image_ms_min_max": [round(imaged[0], 3), round(imaged[-1], 3)],
            "added_ms": round(med(imaged) - med(plain), 3)},
})
print(line, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
