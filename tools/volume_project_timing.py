"""What the two video views cost on BASELINE config 5's filled 10 GB grid, measured on one GPU in one process:
r3d_volume_project with both views, with the above view only and with the elevation view only, beside
r3d_volume_compact over the whole grid (the yardstick: it streams the same 10 GB once).
    python tools/volume_project_timing.py [histories=12500000] [toa_degree=9] [frame_group=1]
HIP events around the launches, 2 warm-up calls, median and range of 5."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from radiative3d_amd import Model, Engine, _ffi
from radiative3d_amd.configs import crustpinch_vids, CRUSTPINCH_VOLUME
from radiative3d_amd.model import project_volume, range_bins
from radiative3d_amd.parallel import DeviceVolume, DeviceResult

n = int(sys.argv[1]) if len(sys.argv) > 1 else 12_500_000
deg = int(sys.argv[2]) if len(sys.argv) > 2 else 9
group = int(sys.argv[3]) if len(sys.argv) > 3 else 1
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


outs = {}
def both():  outs["both"] = project_volume(vol.counters, vol.desc, 0, nf, group, rb, n_range, True, outs.get("both"))
def above(): outs["above"] = project_volume(vol.counters, vol.desc, 0, nf, group, None, 0, True, outs.get("above"))
def elev():  outs["elev"] = project_volume(vol.counters, vol.desc, 0, nf, group, rb, n_range, False, outs.get("elev"))

pairs = torch.empty((1, 2), dtype=torch.int32, device="cuda:0")
n_dev = torch.zeros(1, dtype=torch.int64, device="cuda:0")
def compact():   # (no room to write: the pairs are counted, the grid is streamed once)
    assert lib.r3d_volume_compact(0, vol.counters.data_ptr(), 0, cells, pairs.data_ptr(), 0, n_dev.data_ptr(), stream) == 0

print(f"config 5: {n} histories, {vol.total()} events binned, {nonzero} of {cells} cells non-zero "
      f"({100.0 * nonzero / cells:.2f} %); frame_group {group}, n_range {n_range}, dr {dr:.4f} km")
base = None
for name, call in (("r3d_volume_compact, whole grid", compact), ("r3d_volume_project, both views", both),
                   ("r3d_volume_project, above only", above), ("r3d_volume_project, elevation only", elev),
                   ("r3d_volume_compact, whole grid (again)", compact)):
    med, lo, hi = timed(call)
    base = base or med
    print(f"  {name:40s} median {med:8.3f} ms (range {lo:.3f} - {hi:.3f}) = {4 * cells / med / 1e6:6.0f} GB/s of grid read, "
          f"{med / base:.2f} x the compaction")
vol.detach(); e.close()
