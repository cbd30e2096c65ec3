"""What standard errors cost a job sharded over devices: one JSON line.

    python tools/shard_stats_timing.py [config] [toa-degree] [histories] [batches] [devices]     (crustpinch 9 10000000 16 0,0)

(i)  wall time of Node(devices).run_batched(n, N) (r3d_node_run_batched: N / D batches per shard, a shard's half of the
     moments on its device, the states copied to shard 0's, the merge, the read-back) against Engine.run_batched(n, N)
     (r3d_run_batched: the same N batches on one engine), same build, same process, interleaved on fresh ids;
(ii) the merge kernels alone (r3d_batch_merge over D shard states of the model's block size) against a device-to-device
     copy of the bytes they read, with the GB/s of each.
A warm-up first, then `reps` timed repetitions: the host clock around the synchronous runs, hipEvents for the kernels;
medians and the spread are reported."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from radiative3d_amd import Engine, Model, Node, _ffi, batch_merge  # noqa: E402
from radiative3d_amd.configs import CONFIGS  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "crustpinch"
deg = int(sys.argv[2]) if len(sys.argv) > 2 else 9
n = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
N = int(sys.argv[4]) if len(sys.argv) > 4 else 16
devices = [int(d) for d in (sys.argv[5] if len(sys.argv) > 5 else "0,0").split(",")]
reps, seed = 5, 0x5EED

model = Model(CONFIGS[name](deg) + ["--device-tables"])
engine = Engine(model)
node = Node(model, devices)
D, B = len(devices), N // len(devices)


def wall_ms(fn, first):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(first)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


one_engine = lambda first: engine.run_batched(n, N, first_id=first, seed=seed)   # noqa: E731
sharded = lambda first: node.run_batched(n, N, first_id=first, seed=seed)        # noqa: E731
one_engine(1 << 40), sharded(1 << 40)
one, many = [], []
for r in range(reps):
    first = (r + 1) * n
    one.append(wall_ms(one_engine, first))
    many.append(wall_ms(sharded, first))

# (ii) the merge over D states of the model's block
dev = torch.device("cuda", devices[0])
shape_e = (model.n_seismometers, model.n_bins, _ffi.R3D_N_ENERGY)
shape_c = (model.n_seismometers, model.n_bins, _ffi.R3D_N_COUNT)
es = torch.rand((D,) + shape_e, dtype=torch.float64, device=dev)
ess = torch.rand((D,) + shape_e, dtype=torch.float64, device=dev)
cs = torch.randint(0, 1000, (D,) + shape_c, dtype=torch.int64, device=dev)
css = torch.rand((D,) + shape_c, dtype=torch.float64, device=dev)
energy = torch.zeros(shape_e, dtype=torch.float64, device=dev)
counts = torch.zeros(shape_c, dtype=torch.int64, device=dev)
copies = [torch.empty_like(t) for t in (es, ess, cs, css)]
bytes_in = sum(t.numel() * 8 for t in (es, ess, cs, css))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def merge():
    batch_merge(es, ess, cs, css, B, energy=energy, counts=counts)


def copy():
    for dst, src in zip(copies, (es, ess, cs, css)):
        dst.copy_(src, non_blocking=True)


merge(), copy(), torch.cuda.synchronize()
mrg = sorted(event_ms(merge) for _ in range(4 * reps))
cpy = sorted(event_ms(copy) for _ in range(4 * reps))

med = statistics.median
print(json.dumps({
    "config": name, "toa_degree": deg, "histories": n, "batches": N, "devices": devices, "reps": reps,
    "one_engine_ms": round(med(one), 3), "one_engine_ms_min_max": [round(min(one), 3), round(max(one), 3)],
    "node_ms": round(med(many), 3), "node_ms_min_max": [round(min(many), 3), round(max(many), 3)],
    "node_over_one_engine": round(med(many) / med(one), 4),
    "block_bytes": energy.numel() * 8 + counts.numel() * 8,
    "merge_bytes_in": bytes_in, "merge_ms": round(med(mrg), 4), "merge_ms_min": round(mrg[0], 4),
    "merge_GBps": round(bytes_in / med(mrg) / 1e6, 1),
    "copy_ms": round(med(cpy), 4), "copy_GBps_read": round(bytes_in / med(cpy) / 1e6, 1),
    "merge_over_copy": round(med(mrg) / med(cpy), 3),
}), flush=True)
node.close()
engine.close()
