"""The scatter-event grid reduced along time on the GPU (include/r3d.h r3d_volume_time_maps): synthetic grids in
caller-owned torch tensors against the numpy definition of tests/volume_maps_cases.py, real runs against the maps of
the grid they filled, and the host-level call over two shards.  Everything compared is an integer, so every
comparison is ==."""
import ctypes as C

import numpy as np
import pytest

from volume_maps_cases import NEVER, SHAPES, frame_ranges, grids_of, neutral_maps, random_grid, tie_grid, time_maps_numpy
from volume_views_cases import grid_desc

pytestmark = pytest.mark.gpu

VIDEO = ("--overridemfp=25,50", "--nodeflect", "--timetolive=350")
GRID = dict(origin=(-200.0, -600.0, -130.0), cell_size=(20.0, 20.0, 10.0), dims=(64, 60, 14), n_frames=35, frame_dt=10.0)
CANARY32, CANARY64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def _dev(a):
    import torch
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}[a.dtype]
    return torch.from_numpy(np.ascontiguousarray(a).view(signed)).to("cuda:0")


def _host(maps):
    """The four device maps as numpy uint32 / uint64 (None stays None)."""
    kinds = (np.uint32, np.uint32, np.uint32, np.uint64)
    return tuple(None if t is None else t.cpu().numpy().view(k) for t, k in zip(maps, kinds))


def _maps(grid_dev, desc, f0, f1, min_count=1, outputs=None, **which):
    import torch
    from radiative3d_amd.model import time_maps_volume
    out = time_maps_volume(grid_dev, desc, f0, f1, min_count, outputs=outputs, **which)
    torch.cuda.synchronize()
    return out


def _same(got, want):
    return all((g == w).all() and g.dtype == w.dtype for g, w in zip(got, want))


@pytest.mark.parametrize("shape", SHAPES)
def test_all_maps_equal_numpy(shape):
    nx, ny, nz, nf = shape
    desc = grid_desc(shape)
    for name, grid in grids_of(shape, nx + 100 * nf):
        g = _dev(grid)
        for min_count in (1, 3):
            for f0, f1 in frame_ranges(nf) + ((nf // 2, nf // 2),):
                got = _host(_maps(g, desc, f0, f1, min_count))
                assert _same(got, time_maps_numpy(grid, f0, f1, min_count)), (name, min_count, f0, f1)
                if f0 == f1:                                           # an empty range: a success that touches nothing
                    assert _same(got, neutral_maps(grid))
        assert (g.cpu().numpy().view(np.uint32) == grid).all()         # the grid is only read


def test_a_grid_that_is_not_16_byte_aligned_gives_the_same_maps():
    import torch
    shape = (64, 64, 16, 12)
    grid = random_grid(shape, np.random.default_rng(11), 0.2)
    desc = grid_desc(shape)
    want = time_maps_numpy(grid, 0, 12, 2)
    aligned = _host(_maps(_dev(grid), desc, 0, 12, 2))
    buf = torch.zeros(grid.size + 1, dtype=torch.int32, device="cuda:0")
    buf[1:] = _dev(grid).reshape(-1)
    assert buf[1:].data_ptr() % 16 == 4
    offset = _host(_maps(buf[1:], desc, 0, 12, 2))
    assert _same(aligned, want) and _same(offset, want)


@pytest.mark.parametrize("shape", ((13, 16, 9, 17), (64, 64, 16, 12)))
def test_each_subset_of_the_maps_alone(shape):
    grid = tie_grid(shape, np.random.default_rng(3), 0.6)
    desc = grid_desc(shape)
    g = _dev(grid)
    full = _host(_maps(g, desc, 1, shape[3], 2))
    assert _same(full, time_maps_numpy(grid, 1, shape[3], 2))
    for which, kept in ((dict(first=False, peak=False), (3,)), (dict(peak=False, total=False), (0,)),
                        (dict(first=False, total=False), (1, 2))):
        got = _host(_maps(g, desc, 1, shape[3], 2, **which))
        for k in range(4):
            assert (got[k] is None) == (k not in kept), (which, k)
            if k in kept:
                assert (got[k] == full[k]).all(), (which, k)


def test_pieces_in_reverse_order_update_to_the_maps_of_one_call_and_repeat_to_the_bit():
    shape = (64, 64, 16, 12)
    rng = np.random.default_rng(5)
    desc = grid_desc(shape)
    for grid in (random_grid(shape, rng, 0.05), tie_grid(shape, rng, 0.6)):
        g = _dev(grid)
        want = time_maps_numpy(grid, 0, 12, 1)
        one = _host(_maps(g, desc, 0, 12))
        assert _same(one, want)
        runs = []
        for _ in range(2):
            for k in (1, 5, 8, 11):
                maps = _maps(g, desc, k, 12)
                again = _maps(g, desc, 0, k, outputs=maps)                 # UPDATED: the same tensors
                assert all(a is b for a, b in zip(again, maps))
                runs.append(_host(maps))
                assert _same(runs[-1], want), k
        for a, b in zip(runs[:4], runs[4:]):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))  # the same bits on every run
        assert (g.cpu().numpy().view(np.uint32) == grid).all()             # the grid is only read


def test_a_cell_at_the_ceiling_in_several_frames():
    shape = (64, 64, 16, 12)
    grid = random_grid(shape, np.random.default_rng(9), 0.05)
    top = 0xFFFFFFFF
    grid[0, :, 3, 10, 21] = 0
    grid[0, (4, 7, 9), 3, 10, 21] = top
    grid[0, 2, 3, 10, 21] = top - 1
    grid[1, :, 15, 63, 63] = top                                           # every frame, the grid's last cell
    first, peak_frame, peak_count, total = _host(_maps(_dev(grid), grid_desc(shape), 0, 12, 1))
    assert peak_count[0, 3, 10, 21] == top and peak_frame[0, 3, 10, 21] == 4 and first[0, 3, 10, 21] == 2
    assert int(total[0, 3, 10, 21]) == 3 * top + top - 1
    assert peak_count[1, 15, 63, 63] == top and peak_frame[1, 15, 63, 63] == 0 and int(total[1, 15, 63, 63]) == 12 * top
    assert _same((first, peak_frame, peak_count, total), time_maps_numpy(grid, 0, 12, 1))


def test_every_refusal_leaves_the_outputs_as_they_were():
    import torch
    from radiative3d_amd import _ffi
    L = _ffi.hip_lib()
    shape = (13, 16, 9, 17)
    desc = grid_desc(shape)
    grid = random_grid(shape, np.random.default_rng(1), 0.3)
    g = _dev(grid)
    u32 = [torch.full((2, 9, 16, 13), CANARY32, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    u64 = torch.full((2, 9, 16, 13), CANARY64, dtype=torch.int64, device="cuda:0")

    def untouched():
        return all((t == CANARY32).all() for t in u32) and (u64 == CANARY64).all()

    def call(grid=g.data_ptr(), d=desc, none=False, **kw):
        base = dict(size=C.sizeof(_ffi.VolumeMaps), frame_begin=0, frame_end=17, min_count=1, d_first=u32[0].data_ptr(),
                    d_peak_frame=u32[1].data_ptr(), d_peak_count=u32[2].data_ptr(), d_total=u64.data_ptr())
        base.update(kw)
        m = _ffi.VolumeMaps(**base)
        rc = L.r3d_volume_time_maps(0, grid, C.byref(d) if d is not None else None, None if none else C.byref(m), None)
        torch.cuda.synchronize()
        return rc, L.r3d_last_error().decode()

    for kw, match in ((dict(grid=None), "null"), (dict(d=None), "null"), (dict(none=True), "null"),
                      (dict(size=C.sizeof(_ffi.VolumeMaps) - 8), "size"), (dict(frame_begin=6, frame_end=5), "before frame_begin"),
                      (dict(frame_end=18), "beyond the grid"), (dict(min_count=0), "min_count 0"),
                      (dict(d_first=None, d_peak_frame=None, d_peak_count=None, d_total=None), "no map"),
                      (dict(d_peak_frame=None), "both or neither"), (dict(d_peak_count=None), "both or neither")):
        rc, msg = call(**kw)
        assert rc != 0 and match in msg, (kw, msg)
        assert untouched(), kw
    rc, _ = call(frame_begin=4, frame_end=4)                  # an empty range: success, nothing touched
    assert rc == 0 and untouched()
    for t in u32[:2]:
        t.fill_(-1)
    u32[2].zero_(), u64.zero_()
    rc, _ = call()                                            # and the call that is in order goes through
    assert rc == 0
    assert _same(_host((u32[0], u32[1], u32[2], u64)), time_maps_numpy(grid, 0, 17, 1))


def test_maps_of_a_real_runs_grid(models):
    """A tetra model with a grid attached: the maps of the ENGINE's grid (r3d_volume_device_ptr) equal the numpy maps of
    what r3d_volume_read returns; the totals are the grid's; no cell peaks before it is first reached."""
    import torch
    from radiative3d_amd import Engine, _ffi
    from radiative3d_amd.model import neutral_time_maps, volume_desc
    m = models("crustpinch", 4, VIDEO)
    desc = volume_desc(**GRID)
    e = Engine(m)
    e.set_volume(**GRID)
    r = e.run(20000)
    host = e.read_volume()
    nf = GRID["n_frames"]
    L = _ffi.hip_lib()
    for min_count in (1, 2):
        maps = neutral_time_maps(desc, "cuda:0")
        v = _ffi.VolumeMaps(size=C.sizeof(_ffi.VolumeMaps), frame_begin=0, frame_end=nf, min_count=min_count,
                            d_first=maps[0].data_ptr(), d_peak_frame=maps[1].data_ptr(), d_peak_count=maps[2].data_ptr(),
                            d_total=maps[3].data_ptr())
        assert L.r3d_volume_time_maps(0, e.volume_device_ptr(), C.byref(desc), C.byref(v), None) == 0, L.r3d_last_error()
        torch.cuda.synchronize()
        first, peak_frame, peak_count, total = got = _host(maps)
        assert _same(got, time_maps_numpy(host, 0, nf, min_count))
        assert int(total.sum()) == int(host.sum(dtype=np.uint64)) == r.events["scatter"] + r.events["reflect"] - r.events["volume_out"] > 1000
        seen = peak_count > 0
        assert seen.sum() > 100 and ((peak_frame != NEVER) == seen).all()
        if min_count == 1:
            assert ((first != NEVER) == seen).all() and (first[seen] <= peak_frame[seen]).all()
        else:
            assert ((first != NEVER) == (peak_count >= 2)).all() and (first == NEVER)[seen].any()
    assert (e.read_volume() == host).all()
    e.close()


def test_two_shards_on_one_gpu_merge_their_own_frames_on_the_host(models):
    """devices = 0, 0: two engines run the halves of a job, r3d_volume_reduce_by_frame leaves each with the job's counts
    for its frames; r3d_volume_time_maps_to_host over each engine's OWN frames, into one set of host arrays, in either
    order of the engines, equals numpy on the grid of one engine that ran all ids.  And DeviceVolume.time_maps
    refuses frames that are not the owner's."""
    from radiative3d_amd import Engine, _ffi
    from radiative3d_amd.model import reduce_volumes_by_frame, volume_desc
    from radiative3d_amd.parallel import DeviceVolume
    m = models("crustpinch", 4, VIDEO)
    desc = volume_desc(**GRID)
    nf = GRID["n_frames"]
    n = 24000
    one = Engine(m)
    one.set_volume(**GRID)
    one.run(n)
    whole = one.read_volume()
    one.close()
    engines, vols = [], []
    for lo, hi in ((0, n // 2), (n // 2, n)):
        e = Engine(m, device=0)
        vols.append(DeviceVolume(e, device="cuda:0", **GRID))
        e.run(hi - lo, first_id=lo)
        engines.append(e)
    frames, sat = reduce_volumes_by_frame(engines)
    assert frames == [0, 18, 35] and sat == 0
    L = _ffi.hip_lib()
    for min_count in (1, 2):
        want = time_maps_numpy(whole, 0, nf, min_count)
        for order in ((0, 1), (1, 0)):
            first, peak_frame, peak_count, total = maps = neutral_maps(whole)
            for g in order:
                assert L.r3d_volume_time_maps_to_host(0, engines[g].volume_device_ptr(), C.byref(desc), frames[g], frames[g + 1],
                                                      min_count, first.ctypes.data, peak_frame.ctypes.data,
                                                      peak_count.ctypes.data, total.ctypes.data) == 0, L.r3d_last_error()
            assert _same(maps, want), (min_count, order)
        only_total = np.zeros_like(want[3])
        for g in (0, 1):
            assert L.r3d_volume_time_maps_to_host(0, engines[g].volume_device_ptr(), C.byref(desc), frames[g], frames[g + 1],
                                                  min_count, None, None, None, only_total.ctypes.data) == 0
        assert (only_total == want[3]).all()
    for g, v in enumerate(vols):
        v.owned = (frames[g], frames[g + 1])
        with pytest.raises(RuntimeError, match="hold job totals"):
            v.time_maps(0, nf)
    got = None
    for v in vols:
        got = v.time_maps(outputs=got)
    import torch
    torch.cuda.synchronize()
    assert _same(_host(got), time_maps_numpy(whole, 0, nf, 1))
    for v, e in zip(vols, engines):
        v.detach()
        e.close()
