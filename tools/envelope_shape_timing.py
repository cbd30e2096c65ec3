"""What the envelope shape costs next to the batched run it follows, and next to making it on the host: one JSON line.

    python tools/envelope_shape_timing.py [out.json] [histories]          (none, 10000000)

Crust-pinch model at TOA degree 9, B = 16 batches, the array all 480 receivers, every receiver's window from the default
phase edge to the end of the trace (Model.envshape_plan), SMOOTH 8, weights 1, 1, 1.  Medians of 5 after a warm-up, with
the spread.
(a) the run: Engine.run_batched_envelope_shape against Engine.run_batched of the same ids, wall clock: what the shape adds
    to a run that has to be made anyway, per call and as a share of it.
(b) the kernels alone (r3d_envelope_shape with every output, and with the six numbers only) on the kept blocks of such a run,
    by device events around `inner` launches: milliseconds, the bytes of the blocks they read (40 per window bin and batch)
    and the rate that gives -- against a device-to-device copy of as many bytes, the yardstick that is not the code under
    test.
(c) the alternative it replaces: the B kept blocks copied to the host (wall clock), plus the header's own host build
    (radiative3d_amd/shapes/r3d_envelope_shape.h compiled here by g++ -O2, one thread) on them.
No threshold is asserted anywhere."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radiative3d_amd import Engine, Model, envelope_shape  # noqa: E402
from radiative3d_amd.configs import CONFIGS  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
B, reps, inner, seed, smooth = 16, 5, 20, 0x5EED, 8
WEIGHTS = (1.0, 1.0, 1.0, 0.0, 0.0)
dev = torch.device("cuda", 0)
med = statistics.median

HOST = r'''
#include "r3d_envelope_shape.h"
using namespace r3d;
extern "C" void shape_host(const double* x, uint32_t B, uint32_t S, uint32_t n_bins, uint32_t smooth, const uint32_t* bins,
                           const double* w, double* shape, double* shape_se, double* envelope, double* envelope_se) {
  EnvelopeProblem a;
  a.x = x, a.n_batches = B, a.n_seismometers = S, a.n_bins = n_bins, a.first = 0, a.last = S - 1, a.smooth = smooth, a.bins = bins;
  for (int c = 0; c < 5; c++) a.weight[c] = w[c];
  envelope_shape<1>(a, shape, shape_se, envelope, envelope_se, nullptr, nullptr, nullptr, nullptr);
}
'''


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
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return [event_ms(fn) for _ in range(reps)]


model = Model(CONFIGS["crustpinch"](9))
S, n_bins = model.n_seismometers, model.n_bins
assert S == 480
_, bins, _ = model.envshape_plan(dict(first=0, last=S - 1))
window_bins = int((bins[:, 1].astype(np.int64) - bins[:, 0]).sum())
read_bytes = B * window_bins * 40

# (a) the run
e = Engine(model)
plain = wall(lambda: e.run_batched(n, B, seed=seed))
shaped = wall(lambda: e.run_batched_envelope_shape(n, B, bins, 0, S - 1, WEIGHTS, smooth, seed=seed))
added = med(shaped) - med(plain)

# (b) the kernels alone, on the kept blocks of such a run
be = e.run_batched(n, B, seed=seed, keep_batches=True)[3]
e.close()
dbe = torch.from_numpy(be).to(dev)
dbins = torch.from_numpy(bins.view(np.int32)).to(dev)
src = torch.empty(read_bytes // 8, dtype=torch.int64, device=dev).random_()
dst = torch.empty_like(src)
copy = timed(lambda: dst.copy_(src, non_blocking=True))
everything = timed(lambda: envelope_shape(dbe, dbins, 0, S - 1, WEIGHTS, smooth))
numbers_only = timed(lambda: envelope_shape(dbe, dbins, 0, S - 1, WEIGHTS, smooth, with_envelope=False))
no_se = timed(lambda: envelope_shape(dbe, dbins, 0, S - 1, WEIGHTS, smooth, with_se=False))


def kernel_entry(t):
    return dict(spread(t), gb_per_s=round(read_bytes / (med(t) * 1e-3) / 1e9, 1), over_copy=round(med(t) / med(copy), 2))


# (c) the blocks to the host, and the header's host build on them
host_blocks = torch.empty(dbe.shape, dtype=torch.float64)


def to_host():
    host_blocks.copy_(dbe)
    torch.cuda.synchronize()


d2h = wall(to_host)
with tempfile.TemporaryDirectory(prefix="envelope_shape_timing_") as tmp:
    with open(os.path.join(tmp, "wrap.cpp"), "w") as f:
        f.write(HOST)
    lib = os.path.join(tmp, "libshape_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I",
                           os.path.join(REPO, "radiative3d_amd", "shapes"), "-o", lib, os.path.join(tmp, "wrap.cpp")])
    L = C.CDLL(lib)
    L.shape_host.argtypes = [C.c_void_p] + [C.c_uint32] * 4 + [C.c_void_p] * 6
    L.shape_host.restype = None
    w = np.array(WEIGHTS)
    b = np.ascontiguousarray(bins, dtype=np.uint32)
    hs, hse = np.zeros((S, 6)), np.zeros((S, 6))
    henv, henv_se = np.zeros((S, n_bins)), np.zeros((S, n_bins))
    host = wall(lambda: L.shape_host(be.ctypes.data, B, S, n_bins, smooth, b.ctypes.data, w.ctypes.data, hs.ctypes.data,
                                     hse.ctypes.data, henv.ctypes.data, henv_se.ctypes.data))
got = envelope_shape(dbe, dbins, 0, S - 1, WEIGHTS, smooth)
torch.cuda.synchronize()
same = bool((got["shape"].cpu().numpy().view(np.int64) == hs.view(np.int64)).all()
            and (got["shape_se"].cpu().numpy().view(np.int64) == hse.view(np.int64)).all())

line = json.dumps({
    "config": "crustpinch", "toa_degree": 9, "histories": n, "batches": B, "receivers": S, "bins": n_bins, "smooth": smooth,
    "weights": WEIGHTS, "reps": reps, "launches_per_sample": inner, "window_bins": window_bins, "blocks_bytes_read": read_bytes,
    "run": {"run_batched": spread(plain), "run_batched_envelope_shape": spread(shaped), "added_ms_per_call": round(added, 3),
            "added_share_of_run": round(added / med(plain), 5)},
    "kernel": {"copy_of_as_many_bytes": spread(copy), "all_outputs": kernel_entry(everything),
               "six_numbers_and_se_only": kernel_entry(numbers_only), "without_se": kernel_entry(no_se)},
    "host_alternative": {"blocks_to_host": spread(d2h), "blocks_bytes": int(be.nbytes), "host_build_one_thread": spread(host),
                         "total_ms": round(med(d2h) + med(host), 3), "same_bits_as_the_kernel": same},
})
print(line, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
