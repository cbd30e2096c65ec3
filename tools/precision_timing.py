"""What a run to a target standard error costs beyond its traversal: one JSON line.

    python tools/precision_timing.py [config] [toa-degree] [round-histories] [rounds] [batches] [out.json]
                                                                              (crustpinch 9 10000000 8 16)

The target is unreachable (REL the smallest normal double, COVERAGE 1), so all R rounds run.
(i)   the whole r3d_run_to_precision call -- its allocation, R rounds, the final read-back -- on the host clock, against
      R back-to-back r3d_run_device_batched calls of the same ids with ONE synchronise at the end, same process,
      alternating: that is the path a caller had before this call existed.  Their difference over R is what a round
      pays for being judged.
(ii)  where it goes: the same rounds driven from here through the device-level calls, per round the traversal
      (r3d_run_device_batched, device events), partial + merge + judge (device events), the synchronise and the read-back
      of the judge's four numbers (host clock), the round's wall time, and the idle gap = wall - the two device spans:
      what the device waits for the host between a judge and the next round's first launch.  (Driven through ctypes this
      gap holds Python's call overhead too: an upper bound of the C loop's.)
(iii) the judge alone (device events), and the bytes it reads.
Warm-up first, then `reps` repetitions; medians with min and max."""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from radiative3d_amd import Engine, Model, _ffi, precision_judge  # noqa: E402
from radiative3d_amd.configs import CONFIGS  # noqa: E402
from radiative3d_amd.model import precision_spec  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "crustpinch"
deg = int(sys.argv[2]) if len(sys.argv) > 2 else 9
m = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
R = int(sys.argv[4]) if len(sys.argv) > 4 else 8
B = int(sys.argv[5]) if len(sys.argv) > 5 else 16
out_path = sys.argv[6] if len(sys.argv) > 6 else None
reps, seed = 5, 0x5EED
TINY = float(np.finfo(np.float64).tiny)

model = Model(CONFIGS[name](deg) + ["--device-tables"])
e = Engine(model)
L = e._lib
dev = torch.device("cuda", 0)
S, nb = model.n_seismometers, model.n_bins
ne, nc = S * nb * _ffi.R3D_N_ENERGY, S * nb * _ffi.R3D_N_COUNT
f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)   # noqa: E731
i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)     # noqa: E731
energy, counts, scalars, ese, cse = f64(S, nb, 5), i64(S, nb, 2), i64(_ffi.R3D_N_SCALARS), f64(S, nb, 5), f64(S, nb, 2)
own_e, own_c = f64(ne), i64(nc)
be, bc = f64(B, ne), i64(B, nc)
s_e, ss_e, s_c, ss_c = f64(R, ne), f64(R, ne), i64(R, nc), f64(R, nc)
judged = i64(4 + 4 * S)                                      # totals [3], worst [1], rows [S][3], worst rows [S]
outputs = (judged[4:4 + 3 * S].view(S, 3), judged[4 + 3 * S:].view(torch.float64), judged[:3], judged[3:4].view(torch.float64))
stream = torch.cuda.current_stream(dev)
raw = stream.cuda_stream
spec = precision_spec(S, nb, 0, S - 1, rel=TINY, coverage=1.0)


def check(rc):
    if rc:
        raise RuntimeError(L.r3d_last_error().decode())


def wall_ms(fn, first):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(first)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def whole_call(first):
    res = model.new_result()
    rep = _ffi.PrecisionReport()
    rep.size = C.sizeof(rep)
    c = res._as_c()
    check(L.r3d_run_to_precision(e._e, R * m, first, seed, B, R, C.byref(spec), C.byref(c), None, None, C.byref(rep)))
    assert rep.rounds == R and not rep.met and rep.histories == R * m


def back_to_back(first):
    for g in range(R):
        check(L.r3d_run_device_batched(e._e, m, first + g * m, seed, B, energy.data_ptr(), counts.data_ptr(), scalars.data_ptr(),
                                       ese.data_ptr(), cse.data_ptr(), be.data_ptr(), bc.data_ptr(), raw))


def event():
    return torch.cuda.Event(enable_timing=True)


def driven_rounds(first):
    """The call's loop through the device-level entry points: per round (traversal, stats, sync + read-back, wall) ms."""
    rows = []
    for g in range(R):
        a, b, c = event(), event(), event()
        t0 = time.perf_counter()
        a.record(stream)
        check(L.r3d_run_device_batched(e._e, m, first + g * m, seed, B, own_e.data_ptr(), own_c.data_ptr(), scalars.data_ptr(),
                                       None, None, be.data_ptr(), bc.data_ptr(), raw))
        b.record(stream)
        check(L.r3d_batch_partial(0, B, be.data_ptr(), ne, bc.data_ptr(), nc, None, 0, s_e[g].data_ptr(), ss_e[g].data_ptr(),
                                  s_c[g].data_ptr(), ss_c[g].data_ptr(), None, raw))
        energy.zero_(), counts.zero_()
        check(L.r3d_batch_merge(0, g + 1, B, s_e.data_ptr(), ss_e.data_ptr(), ne, s_c.data_ptr(), ss_c.data_ptr(), nc, None, 0,
                                energy.data_ptr(), counts.data_ptr(), None, ese.data_ptr(), cse.data_ptr(), raw))
        precision_judge(energy, ese, counts, 0, S - 1, rel=TINY, coverage=1.0, outputs=outputs)
        c.record(stream)
        stream.synchronize()
        t1 = time.perf_counter()
        four = judged[:4].cpu()
        t2 = time.perf_counter()
        assert int(four[0]) >= int(four[1])
        rows.append((a.elapsed_time(b), b.elapsed_time(c), (t2 - t1) * 1e3, (t2 - t0) * 1e3))
    return rows


# warm-up: every shape the timed window uses
whole_call(1 << 40), back_to_back(1 << 40), driven_rounds(1 << 40), torch.cuda.synchronize()
call, plain, rounds = [], [], []
for r in range(reps):
    first = (r + 1) * R * m
    plain.append(wall_ms(back_to_back, first))
    call.append(wall_ms(whole_call, first))
    torch.cuda.synchronize()
    rounds += driven_rounds(first)
torch.cuda.synchronize()


def judge_ms():
    a, b = event(), event()
    a.record(stream)
    precision_judge(energy, ese, counts, 0, S - 1, rel=TINY, coverage=1.0, outputs=outputs)
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


judge = sorted(judge_ms() for _ in range(4 * reps))
med = statistics.median
trav, stats, readback, wall = (med([row[k] for row in rounds]) for k in range(4))   # (over every round of every repetition)
per_round = (med(call) - med(plain)) / R
line = {
    "config": name, "toa_degree": deg, "seismometers": S, "bins": nb, "round_histories": m, "rounds": R, "batches": B,
    "reps": reps,
    "precision_call_ms": round(med(call), 3), "precision_call_ms_min_max": [round(min(call), 3), round(max(call), 3)],
    "back_to_back_ms": round(med(plain), 3), "back_to_back_ms_min_max": [round(min(plain), 3), round(max(plain), 3)],
    "call_over_back_to_back": round(med(call) / med(plain), 4),
    "overhead_per_round_ms": round(per_round, 4), "overhead_per_round_pct": round(100 * per_round / (med(plain) / R), 2),
    "driven_round_wall_ms": round(wall, 4), "driven_traversal_ms": round(trav, 4),
    "driven_partial_merge_judge_ms": round(stats, 4), "driven_sync_readback_ms": round(readback, 4),
    "driven_idle_gap_ms": round(wall - trav - stats, 4),
    "driven_partial_merge_judge_ms_first_last_round": [round(med([rounds[i][1] for i in range(0, len(rounds), R)]), 4),
                                                       round(med([rounds[i][1] for i in range(R - 1, len(rounds), R)]), 4)],
    "judge_ms": round(med(judge), 4), "judge_ms_min": round(judge[0], 4),
    "judge_bytes_read": (2 * ne + nc) * 8, "judge_GBps": round((2 * ne + nc) * 8 / med(judge) / 1e6, 1),
}
text = json.dumps(line)
print(text, flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
e.close()
