"""What per-bin standard errors cost, and how well they are calibrated: one JSON line.

    python tools/batched_run_timing.py [config] [toa-degree] [histories] [batches]     (crustpinch 9 10000000 16)

(i)   wall time of r3d_run_device_batched (B self-contained launches over four streams + the moments kernel)
      against ONE r3d_run_device of the same ids, same build, same process;
(ii)  the moments kernels alone (r3d_batch_moments over the B kept blocks) against a device-to-device hipMemcpyAsync
      of the same B x len bytes -- the yardstick that is not the code under test -- with the GB/s of each;
(iii) calibration: two batched runs of disjoint id ranges, z = (T1 - T2) / sqrt(se1^2 + se2^2) over the P and S
      energy entries of bins with at least 25 catches in both runs; its r.m.s. is 1 for an honest standard error.
Warm-up launches first, then `reps` timed repetitions, hipEvents on the stream for the kernels and the host clock
around a synchronize for the runs; medians and the spread are reported."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radiative3d_amd import Engine, Model, _ffi, batch_moments  # noqa: E402
from radiative3d_amd.configs import CONFIGS  # noqa: E402
from radiative3d_amd.parallel import DeviceResult  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "crustpinch"
deg = int(sys.argv[2]) if len(sys.argv) > 2 else 9
n = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
B = int(sys.argv[4]) if len(sys.argv) > 4 else 16
reps, seed = 5, 0x5EED

model = Model(CONFIGS[name](deg) + ["--device-tables"])
e = Engine(model)
L = e._lib
dev = torch.device("cuda", 0)
total = DeviceResult(model, "cuda:0")
shape_e, shape_c = total.energy.shape, total.counts.shape
ese = torch.zeros(shape_e, dtype=torch.float64, device=dev)
cse = torch.zeros(shape_c, dtype=torch.float64, device=dev)
be = torch.zeros((B,) + tuple(shape_e), dtype=torch.float64, device=dev)
bc = torch.zeros((B,) + tuple(shape_c), dtype=torch.int64, device=dev)
stream = torch.cuda.current_stream(dev).cuda_stream


def single(first):
    e.run_device(n, first, seed, *total.pointers())


def batched(first, keep=True):
    if L.r3d_run_device_batched(e._e, n, first, seed, B, *total.pointers(), ese.data_ptr(), cse.data_ptr(),
                                be.data_ptr() if keep else None, bc.data_ptr() if keep else None, stream):
        raise RuntimeError(L.r3d_last_error().decode())


def wall_ms(fn, first):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(first)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


# (i) interleaved, on fresh ids each time (the same ids for the two forms of one repetition)
single(1 << 40), batched(1 << 40), torch.cuda.synchronize()
one, many, scratch = [], [], []
for r in range(reps):
    first = (r + 1) * n
    one.append(wall_ms(single, first))
    many.append(wall_ms(batched, first))
    scratch.append(wall_ms(lambda f: batched(f, keep=False), first))
kernel_one = e.last_kernel_ms()

# (ii) the moments kernels over the kept blocks against a copy of the same bytes
copy_e, copy_c = torch.empty_like(be), torch.empty_like(bc)
bytes_in = be.numel() * 8 + bc.numel() * 8


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def moments():
    batch_moments(be, bc, energy=total.energy, counts=total.counts)


def copy():
    copy_e.copy_(be, non_blocking=True)
    copy_c.copy_(bc, non_blocking=True)


moments(), copy(), torch.cuda.synchronize()
mom = sorted(event_ms(moments) for _ in range(4 * reps))
cpy = sorted(event_ms(copy) for _ in range(4 * reps))

# (iii) calibration on two disjoint id ranges
r1 = e.run_batched(n, B, first_id=100 * n, seed=seed)
r2 = e.run_batched(n, B, first_id=101 * n, seed=seed)
both = (r1[0].counts >= 25) & (r2[0].counts >= 25)                        # [seis, bin, type]
t1, t2, s1, s2 = r1[0].energy[..., 3:5], r2[0].energy[..., 3:5], r1[1][..., 3:5], r2[1][..., 3:5]
z = (t1[both] - t2[both]) / np.sqrt(s1[both] ** 2 + s2[both] ** 2)
c1, c2 = r1[0].counts.astype(np.float64), r2[0].counts.astype(np.float64)
zc = (c1[both] - c2[both]) / np.sqrt(r1[2][both] ** 2 + r2[2][both] ** 2)

med = statistics.median
print(json.dumps({
    "config": name, "toa_degree": deg, "histories": n, "batches": B, "reps": reps,
    "single_run_ms": round(med(one), 3), "single_run_ms_min_max": [round(min(one), 3), round(max(one), 3)],
    "single_kernel_ms": round(kernel_one, 3),
    "batched_run_ms": round(med(many), 3), "batched_run_ms_min_max": [round(min(many), 3), round(max(many), 3)],
    "batched_run_scratch_ms": round(med(scratch), 3),
    "batched_over_single": round(med(many) / med(one), 4),
    "moments_bytes_in": bytes_in, "moments_ms": round(med(mom), 4), "moments_ms_min": round(mom[0], 4),
    "moments_GBps": round(bytes_in / med(mom) / 1e6, 1),
    "copy_ms": round(med(cpy), 4), "copy_ms_min": round(cpy[0], 4), "copy_GBps_read": round(bytes_in / med(cpy) / 1e6, 1),
    "moments_over_copy": round(med(mom) / med(cpy), 3),
    "z_rms_energy": round(float(np.sqrt(np.mean(z ** 2))), 4), "z_rms_counts": round(float(np.sqrt(np.mean(zc ** 2))), 4),
    "z_entries": int(both.sum()),
}), flush=True)
e.close()
