"""What the maps along time cost on BASELINE config 5's filled 10 GB grid, measured on one GPU in one process:
r3d_volume_time_maps with all four maps and with `total` only, beside r3d_volume_compact with capacity 0 over the same
counters (the yardstick: it streams the same 10 GB once and writes nothing) and r3d_volume_project with both views.
    python tools/volume_maps_timing.py [histories=12500000] [toa_degree=9] [min_count=1]
HIP events around the launches, 2 warm-up calls, median and range of 5; prints one JSON line."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from radiative3d_amd import Model, Engine, _ffi
from radiative3d_amd.configs import crustpinch_vids, CRUSTPINCH_VOLUME
from radiative3d_amd.model import neutral_time_maps, project_volume, range_bins, time_maps_volume
from radiative3d_amd.parallel import DeviceVolume, DeviceResult

n = int(sys.argv[1]) if len(sys.argv) > 1 else 12_500_000
deg = int(sys.argv[2]) if len(sys.argv) > 2 else 9
min_count = int(sys.argv[3]) if len(sys.argv) > 3 else 1
m = Model(crustpinch_vids(deg) + ["--device-tables"]); e = Engine(m)
vol = DeviceVolume(e, device="cuda:0", **CRUSTPINCH_VOLUME)
res = DeviceResult(m, "cuda:0")
e.run_device(n, 0, 0x5EED, *res.pointers()); torch.cuda.synchronize()
lib = _ffi.hip_lib()
cells = vol.counters.numel()
nonzero = int((vol.counters != 0).sum().item())
src = m.desc.source.loc
c = CRUSTPINCH_VOLUME["cell_size"]; o = CRUSTPINCH_VOLUME["origin"]; d = CRUSTPINCH_VOLUME["dims"]
dr = min(c[0], c[1])
far = max(((x - src[0]) ** 2 + (y - src[1]) ** 2) ** 0.5 for x in (o[0], o[0] + c[0] * d[0]) for y in (o[1], o[1] + c[1] * d[1]))
n_range = int(far / dr) + 1
rb = torch.from_numpy(range_bins(vol.desc, (src[0], src[1]), dr, n_range).view("int32")).to("cuda:0")
stream = torch.cuda.current_stream().cuda_stream
nf = CRUSTPINCH_VOLUME["n_frames"]


def timed(call):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[2], ms[0], ms[-1]


# (the maps are updated in place: a repeat of the same frames leaves first and the peak as they are and adds to total)
all_four = neutral_time_maps(vol.desc, "cuda:0")
only_total = neutral_time_maps(vol.desc, "cuda:0", first=False, peak=False)
views = {}
def maps_all():   time_maps_volume(vol.counters, vol.desc, 0, nf, min_count, outputs=all_four)
def maps_total(): time_maps_volume(vol.counters, vol.desc, 0, nf, min_count, first=False, peak=False, outputs=only_total)
def both():       views["both"] = project_volume(vol.counters, vol.desc, 0, nf, 1, rb, n_range, True, views.get("both"))

pairs = torch.empty((1, 2), dtype=torch.int32, device="cuda:0")
n_dev = torch.zeros(1, dtype=torch.int64, device="cuda:0")
def compact():   # (no room to write: the pairs are counted, the grid is streamed once)
    assert lib.r3d_volume_compact(0, vol.counters.data_ptr(), 0, cells, pairs.data_ptr(), 0, n_dev.data_ptr(), stream) == 0

out = dict(tool="volume_maps_timing", histories=n, toa_degree=deg, min_count=min_count, events_binned=vol.total(),
           cells=cells, cells_nonzero=nonzero, grid_bytes=4 * cells, map_cells=all_four[0].numel(), calls={})
for name, call in (("compact_capacity_0", compact), ("time_maps_all_four", maps_all), ("time_maps_total_only", maps_total),
                   ("project_both_views", both), ("compact_capacity_0_again", compact)):
    med, lo, hi = timed(call)
    out["calls"][name] = dict(median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                              grid_read_gb_s=round(4 * cells / med / 1e6, 1))
base = out["calls"]["compact_capacity_0"]["median_ms"]
out["maps_over_compact"] = round(out["calls"]["time_maps_all_four"]["median_ms"] / base, 4)
out["total_only_over_compact"] = round(out["calls"]["time_maps_total_only"]["median_ms"] / base, 4)
out["reached_cells"] = int((all_four[0] != -1).sum().item())
print(json.dumps(out))
vol.detach(); e.close()
