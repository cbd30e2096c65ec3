"""The two video views of the scatter-event grid on the GPU (include/r3d.h r3d_volume_project): synthetic grids in
caller-owned torch tensors against the numpy projection of tests/volume_views_cases.py -- everything compared is an
integer, so every comparison is == --, real runs against the projection of the grid they filled, and the one physical
check, whose bound is the header's: an event sits at its cell's centre, at most half the cell's horizontal diagonal
from where it happened."""
import ctypes as C

import numpy as np
import pytest

from volume_views_cases import OUT, SHAPES, grid_desc, n_out_frames, project_numpy, random_grid, range_bins_numpy

pytestmark = pytest.mark.gpu

VIDEO = ("--overridemfp=25,50", "--nodeflect", "--timetolive=350")
GRID = dict(origin=(-200.0, -600.0, -130.0), cell_size=(20.0, 20.0, 10.0), dims=(64, 60, 14), n_frames=35, frame_dt=10.0)
CANARY = 0x5A5A5A5A5A5A5A5A


def _dev(a):
    import torch
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}[a.dtype]
    return torch.from_numpy(np.ascontiguousarray(a).view(signed)).to("cuda:0")


def _host(t):
    return None if t is None else t.cpu().numpy().view(np.uint64)


def _project(grid_dev, desc, f0, f1, group, rb=None, n_range=0, above=True, outputs=None):
    import torch
    from radiative3d_amd.model import project_volume
    out = project_volume(grid_dev, desc, f0, f1, group, rb, n_range, above, outputs)
    torch.cuda.synchronize()
    return out


def _frame_cases(nf):
    return ((0, nf, 1), (0, nf, 3), (0, nf, nf - 1 if nf % (nf - 1) else nf - 2), (1, nf - 1, 1), (1, nf - 1, 2), (2, 3, 5))


@pytest.mark.parametrize("density", (0.03, 0.7))
@pytest.mark.parametrize("shape", SHAPES)
def test_both_views_equal_the_numpy_projection(shape, density):
    nx, ny, nz, nf = shape
    rng = np.random.default_rng(nx + 100 * nf + int(1000 * density))
    grid = random_grid(shape, rng, density)
    desc = grid_desc(shape)
    n_range = 4 if nx < 64 else 40
    rb = range_bins_numpy(desc, (-20.0, 20.0), 2.5, n_range)
    assert (rb == OUT).any() and (rb != OUT).any()
    g = _dev(grid)
    for f0, f1, group in _frame_cases(nf):
        wa, we, wo = project_numpy(grid, f0, f1, group, rb, n_range)
        a, e, o = _project(g, desc, f0, f1, group, rb, n_range)                     # both views
        assert (_host(a) == wa).all() and (_host(e) == we).all() and (_host(o) == wo).all(), (f0, f1, group)
        a, e, o = _project(g, desc, f0, f1, group)                                  # the above view alone
        assert e is None and o is None and (_host(a) == wa).all(), (f0, f1, group)
        a, e, o = _project(g, desc, f0, f1, group, rb, n_range, above=False)        # the elevation view alone
        assert a is None and (_host(e) == we).all() and (_host(o) == wo).all(), (f0, f1, group)
        # conservation
        for t in range(2):
            assert int(wa[t].sum()) == int(_host(e)[t].sum()) + int(_host(o)[t]) == int(grid[t, f0:f1].sum(dtype=np.uint64))
    assert (g.cpu().numpy().view(np.uint32) == grid).all()                   # the grid is only read


def test_a_grid_the_size_of_a_workgroups_histogram_and_beyond():
    """n_range x nz on both sides of what a workgroup keeps in LDS (64 KB without asking, 144 KB at most; beyond that
    the elevation view adds straight into HBM), on rows of whole quads and on a pointer that is not 16-byte aligned."""
    import torch
    shape = (64, 48, 40, 3)
    rng = np.random.default_rng(77)
    grid = random_grid(shape, rng, 0.1)
    desc = grid_desc(shape, cell=(1.0, 1.0, 1.0))
    for n_range, dr in ((300, 0.25), (700, 0.1), (1100, 0.07)):      # 48 KB, 112 KB, 176 KB of histogram
        rb = range_bins_numpy(desc, (-20.0, 20.0), dr, n_range)
        assert len(np.unique(rb)) > n_range // 8
        wa, we, wo = project_numpy(grid, 0, 3, 2, rb, n_range)
        a, e, o = _project(_dev(grid), desc, 0, 3, 2, rb, n_range)
        assert (_host(a) == wa).all() and (_host(e) == we).all() and (_host(o) == wo).all(), n_range
    # the same grid one counter into a larger buffer: 4 bytes off a 16-byte boundary
    rb = range_bins_numpy(desc, (-20.0, 20.0), 0.25, 300)
    wa, we, wo = project_numpy(grid, 0, 3, 1, rb, 300)
    buf = torch.zeros(grid.size + 1, dtype=torch.int32, device="cuda:0")
    buf[1:] = _dev(grid).reshape(-1)
    a, e, o = _project(buf[1:], desc, 0, 3, 1, rb, 300)
    assert buf[1:].data_ptr() % 16 == 4
    assert (_host(a) == wa).all() and (_host(e) == we).all() and (_host(o) == wo).all()


def test_views_accumulate_leave_the_grid_alone_and_repeat_to_the_bit():
    shape = (64, 64, 16, 12)
    rng = np.random.default_rng(5)
    grid = random_grid(shape, rng, 0.05)
    desc = grid_desc(shape)
    rb = range_bins_numpy(desc, (-20.0, 20.0), 2.5, 40)
    g = _dev(grid)
    for group in (1, 12):                # (12: one output frame, whose grid frames meet in HBM through atomics)
        wa, we, wo = project_numpy(grid, 0, 12, group, rb, 40)
        first = _project(g, desc, 0, 12, group, rb, 40)
        again = _project(g, desc, 0, 12, group, rb, 40)
        for x, y in zip(first, again):
            assert (x == y).all()                                            # the same bits on every run
        twice = _project(g, desc, 0, 12, group, rb, 40, outputs=again)       # ADDED into
        assert twice[0] is again[0]
        assert (_host(twice[0]) == 2 * wa).all() and (_host(twice[1]) == 2 * we).all() and (_host(twice[2]) == 2 * wo).all()
        assert (_host(first[0]) == wa).all()
    assert (g.cpu().numpy().view(np.uint32) == grid).all()                   # the grid is only read


def test_cells_at_the_ceiling_do_not_wrap_either_view():
    """Many cells of one column, and many columns of one range bin, at 2^32 - 1: a 32-bit sum anywhere on the way
    (a register, the LDS histogram) would wrap."""
    shape = (64, 64, 16, 4)
    grid = np.zeros((2, 4, 16, 64, 64), dtype=np.uint32)
    desc = grid_desc(shape)
    rb = range_bins_numpy(desc, (-20.0, 20.0), 2.5, 40)
    ring = rb == np.bincount(rb[rb != OUT]).argmax()                         # the range bin with the most columns
    assert ring.sum() >= 16
    grid[0, 1, :, 10, 20] = 0xFFFFFFFF                                       # one column, every depth
    grid[1, 2, 3][ring] = 0xFFFFFFFF                                         # one range bin at one depth, every column
    grid[0, 3, 5][ring] = 0xFFFFFFFF
    grid[0, 3, 5, 0, 0] = 7
    for group in (1, 4):
        wa, we, wo = project_numpy(grid, 0, 4, group, rb, 40)
        assert wa.max() >= 16 * 0xFFFFFFFF and we.max() >= 16 * 0xFFFFFFFF
        a, e, o = _project(_dev(grid), desc, 0, 4, group, rb, 40)
        assert (_host(a) == wa).all() and (_host(e) == we).all() and (_host(o) == wo).all(), group


def test_every_refusal_leaves_the_outputs_as_they_were():
    import torch
    from radiative3d_amd import _ffi
    L = _ffi.hip_lib()
    shape = (13, 16, 9, 10)
    desc = grid_desc(shape)
    g = _dev(random_grid(shape, np.random.default_rng(1), 0.3))
    rb = _dev(range_bins_numpy(desc, (-20.0, 20.0), 2.5, 5))
    above = torch.full((2, 10, 16, 13), CANARY, dtype=torch.int64, device="cuda:0")
    elev = torch.full((2, 10, 9, 5), CANARY, dtype=torch.int64, device="cuda:0")
    outside = torch.full((2,), CANARY, dtype=torch.int64, device="cuda:0")

    def call(grid=g.data_ptr(), d=desc, none=False, **kw):
        base = dict(size=C.sizeof(_ffi.VolumeViews), frame_begin=0, frame_end=10, frame_group=1, n_range=5,
                    d_range_bin=rb.data_ptr(), d_above=above.data_ptr(), d_elev=elev.data_ptr(), d_outside=outside.data_ptr())
        base.update(kw)
        v = _ffi.VolumeViews(**base)
        rc = L.r3d_volume_project(0, grid, C.byref(d) if d is not None else None, None if none else C.byref(v), None)
        torch.cuda.synchronize()
        return rc, L.r3d_last_error().decode()

    for kw, match in ((dict(grid=None), "null"), (dict(d=None), "null"), (dict(none=True), "null"),
                      (dict(size=C.sizeof(_ffi.VolumeViews) - 8), "size"), (dict(frame_begin=6, frame_end=5), "before frame_begin"),
                      (dict(frame_end=11), "beyond the grid"), (dict(frame_group=0), "frame_group 0"),
                      (dict(d_above=None, d_elev=None, d_outside=None), "neither view"),
                      (dict(d_range_bin=None), "column map"), (dict(n_range=0), "column map"),
                      (dict(d_elev=None), "with that view only")):
        rc, msg = call(**kw)
        assert rc != 0 and match in msg, (kw, msg)
        assert (above == CANARY).all() and (elev == CANARY).all() and (outside == CANARY).all(), kw
    rc, _ = call(frame_begin=4, frame_end=4)                  # an empty range: success, nothing touched
    assert rc == 0 and (above == CANARY).all() and (elev == CANARY).all() and (outside == CANARY).all()
    from radiative3d_amd.model import range_bins
    with pytest.raises(RuntimeError, match="dr must be positive"):
        range_bins(desc, (0.0, 0.0), 0.0, 5)
    rc, _ = call()                                            # and the call that is in order goes through
    assert rc == 0 and not (above == CANARY).all()


def _grid_for(m, name):
    """A grid about the model's source that holds most of a small run's events."""
    if name == "crustpinch":
        return dict(GRID)
    s = m.desc.source.loc
    return dict(origin=(s[0] - 300.0, s[1] - 280.0, s[2] - 60.0), cell_size=(24.0, 20.0, 8.0), dims=(25, 28, 12),
                n_frames=20, frame_dt=6.0)


@pytest.mark.parametrize("name", ("crustpinch", "halfspace"))
def test_views_of_a_real_runs_grid(models, name):
    """A tetra and a layered model with a grid attached: the views of the ENGINE's grid (r3d_volume_device_ptr)
    equal the projection of what r3d_volume_read returns, and their totals are the run's SCT + REF events minus the
    ones that fell outside the grid."""
    import torch
    from radiative3d_amd import Engine, _ffi
    from radiative3d_amd.model import range_bins, volume_desc
    m = models(name, 4, VIDEO if name == "crustpinch" else ())
    grid = _grid_for(m, name)
    desc = volume_desc(**grid)
    e = Engine(m)
    e.set_volume(**grid)
    r = e.run(20000)
    host = e.read_volume()
    nx, ny, nz = grid["dims"]
    nf = grid["n_frames"]
    src = m.desc.source.loc
    dr = min(grid["cell_size"][:2])
    n_range = 12
    rb = range_bins(desc, (src[0], src[1]), dr, n_range, 30.0, 100.0)
    assert (rb == range_bins_numpy(desc, (src[0], src[1]), dr, n_range, 30.0, 100.0)).all() and (rb == OUT).any()
    L = _ffi.hip_lib()
    for group in (1, 4):
        n_out = n_out_frames(0, nf, group)
        above = torch.zeros((2, n_out, ny, nx), dtype=torch.int64, device="cuda:0")
        elev = torch.zeros((2, n_out, nz, n_range), dtype=torch.int64, device="cuda:0")
        outside = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        v = _ffi.VolumeViews(size=C.sizeof(_ffi.VolumeViews), frame_begin=0, frame_end=nf, frame_group=group, n_range=n_range,
                             d_range_bin=_dev(rb).data_ptr(), d_above=above.data_ptr(), d_elev=elev.data_ptr(),
                             d_outside=outside.data_ptr())
        assert L.r3d_volume_project(0, e.volume_device_ptr(), C.byref(desc), C.byref(v), None) == 0, L.r3d_last_error()
        torch.cuda.synchronize()
        wa, we, wo = project_numpy(host, 0, nf, group, rb, n_range)
        assert (_host(above) == wa).all() and (_host(elev) == we).all() and (_host(outside) == wo).all()
        total = r.events["scatter"] + r.events["reflect"] - r.events["volume_out"]
        assert int(wa.sum()) == total > 1000 and int(we.sum()) + int(wo.sum()) == total and int(we.sum()) > 0
    assert (e.read_volume() == host).all()
    e.close()


def test_the_elevation_view_against_the_exact_event_positions(models):
    """The reference's own quantity (vis/scattervid/scattervid_p2p.m:135-148): rho, the horizontal distance of an
    event from the epicentre, per frame.  From the event log (SCT | REF) of the run that filled the grid: per wave
    type the events inside the grid are counted exactly by the views, frame by frame, and for every (type, output
    frame) that holds events the mean rho of the elevation view (bin centres, (ir + 0.5) dr) is within
    0.5 sqrt(c_x^2 + c_y^2) + 0.5 dr of the mean exact rho: half a cell's horizontal diagonal for placing an event at
    its cell's centre (include/r3d.h), half a bin for reading a bin at its centre.  The frame and the cell of an event
    are taken by the kernel's own recipe (csrc/r3d_step.h volume_count: t * (1 / dt), (x - o) * (1 / c), truncated) --
    tests/test_volume_grid.py forms no frame index of its own, it holds the grid against the oracle's, which bins
    the same way (oracle/r3d_oracle.cpp) --, so an event on a frame's edge falls where the grid put it; the exact
    per-frame counts below would show a disagreement."""
    import torch
    from radiative3d_amd import Engine
    from radiative3d_amd.model import range_bins, volume_desc
    from radiative3d_amd.parallel import DeviceVolume
    m = models("crustpinch", 4, VIDEO)
    desc = volume_desc(**GRID)
    e = Engine(m)
    vol = DeviceVolume(e, device="cuda:0", **GRID)
    e.set_event_log(2 | 4, 1 << 20)                      # include/r3d.h R3D_RPT_SCT | R3D_RPT_REF
    r = e.run(20000)
    torch.cuda.synchronize()
    assert e.event_log_count() == r.events["scatter"] + r.events["reflect"] < (1 << 20)
    ev = e.read_event_log()
    o, c, dims = np.array(GRID["origin"]), np.array(GRID["cell_size"]), np.array(GRID["dims"], dtype=np.float64)
    f = ev["time"] * (1.0 / GRID["frame_dt"])
    cell = (ev["loc"] - o[None, :]) * (1.0 / c)[None, :]
    inside = (f >= 0) & (f < GRID["n_frames"]) & (cell >= 0).all(axis=1) & (cell < dims[None, :]).all(axis=1)
    assert int((~inside).sum()) == r.events["volume_out"] > 0
    src = m.desc.source.loc
    rho = np.hypot(ev["loc"][:, 0] - src[0], ev["loc"][:, 1] - src[1])
    dr = 20.0
    far = max(np.hypot(x - src[0], y - src[1]) for x in (o[0], o[0] + c[0] * dims[0]) for y in (o[1], o[1] + c[1] * dims[1]))
    n_range = int(far / dr) + 1
    rb = range_bins(desc, (src[0], src[1]), dr, n_range)
    assert (rb != OUT).all()
    bound = 0.5 * np.sqrt(c[0] ** 2 + c[1] ** 2) + 0.5 * dr
    centres = (np.arange(n_range) + 0.5) * dr
    for group in (1, 3):
        above, elev, outside = (_host(x) for x in vol.project(frame_group=group, range_bin=rb, n_range=n_range))
        assert outside.sum() == 0
        F = (f[inside].astype(np.int64)) // group
        n_out = n_out_frames(0, GRID["n_frames"], group)
        checked, worst = 0, 0.0
        for t in range(2):
            of_type = ev["type"][inside] == t
            want = np.bincount(F[of_type], minlength=n_out)
            assert (above[t].sum(axis=(1, 2)) == want).all() and (elev[t].sum(axis=(1, 2)) == want).all(), t
            for k in np.flatnonzero(want):
                per_bin = elev[t, k].sum(axis=0).astype(np.float64)
                mean_view = (per_bin * centres).sum() / per_bin.sum()
                mean_exact = rho[inside][of_type][F[of_type] == k].mean()
                worst = max(worst, abs(mean_view - mean_exact))
                assert abs(mean_view - mean_exact) <= bound, (t, k, mean_view, mean_exact)
                checked += 1
        print(f"group {group}: {checked} (type, frame) means, worst |view - exact| = {worst:.3f} km, bound {bound:.3f} km")
        assert checked > n_out
    vol.detach()
    e.close()


def test_two_shards_on_one_gpu_project_their_own_frames(models):
    """devices = 0, 0: two engines run the halves of a job, r3d_volume_reduce_by_frame leaves each with the job's
    counts for its frames, each projects those; assembled, the views equal those of one engine that ran all ids --
    also where an output frame straddles the two owners and the partial groups are added."""
    import torch
    from radiative3d_amd import Engine
    from radiative3d_amd.model import range_bins, reduce_volumes_by_frame, volume_desc
    from radiative3d_amd.parallel import DeviceVolume
    m = models("crustpinch", 4, VIDEO)
    desc = volume_desc(**GRID)
    nx, ny, nz = GRID["dims"]
    nf = GRID["n_frames"]
    n = 24000
    src = m.desc.source.loc
    rb, n_range = range_bins(desc, (src[0], src[1]), 20.0, 30), 30
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
    for group in (1, 4):                               # (4: output frame 4 = grid frames 16-19 straddles the owners)
        n_out = n_out_frames(0, nf, group)
        above = np.zeros((2, n_out, ny, nx), dtype=np.uint64)
        elev = np.zeros((2, n_out, nz, n_range), dtype=np.uint64)
        outside = np.zeros(2, dtype=np.uint64)
        for g, v in enumerate(vols):
            v.owned = (frames[g], frames[g + 1])
            with pytest.raises(RuntimeError, match="hold job totals"):
                v.project(0, nf, group, rb, n_range)
            begin, hi = v.owned
            while begin < hi:                          # the owner's frames, cut where the job's groups are cut
                end = min(hi, (begin // group + 1) * group)
                a, el, o = v.project(begin, end, group, rb, n_range)
                torch.cuda.synchronize()
                above[:, begin // group] += _host(a)[:, 0]
                elev[:, begin // group] += _host(el)[:, 0]
                outside += _host(o)
                begin = end
        wa, we, wo = project_numpy(whole, 0, nf, group, rb, n_range)
        assert (above == wa).all() and (elev == we).all() and (outside == wo).all(), group
    for v, e in zip(vols, engines):
        v.detach()
        e.close()


def test_full_size_views_of_the_10_gb_grid():
    """BASELINE config 5 at TOA degree 9 with the 10 GB grid (as test_volume_grid.py's full-size run), both views with
    frame_group 1: the views' totals per wave type equal the grid's and the run's counters, and the above view of a
    fixed sample of 8 frames per type equals torch.sum over z of those frames."""
    import torch
    from radiative3d_amd import Engine, Model
    from radiative3d_amd.configs import CRUSTPINCH_VOLUME, crustpinch_vids
    from radiative3d_amd.model import range_bins
    from radiative3d_amd.parallel import DeviceVolume
    m = Model(crustpinch_vids(9))
    e = Engine(m)
    vol = DeviceVolume(e, device="cuda:0", **CRUSTPINCH_VOLUME)
    n = 10_000_000
    r = e.run(n)
    torch.cuda.synchronize()
    total = r.events["scatter"] + r.events["reflect"] - r.events["volume_out"]
    assert vol.total() == total > 5 * n
    src = m.desc.source.loc
    c = CRUSTPINCH_VOLUME["cell_size"]
    dr = min(c[0], c[1])
    n_range = 150                                            # 1172 km of the 1414 km to the corners, and a cone of
    rb = range_bins(vol.desc, (src[0], src[1]), dr, n_range, 90.0, 60.0)   # azimuths: some columns are outside the view
    assert (rb == OUT).any() and (rb != OUT).any()
    above, elev, outside = vol.project(range_bin=rb, n_range=n_range)
    torch.cuda.synchronize()
    assert above.shape == (2, 300, 256, 256) and elev.shape == (2, 300, 64, n_range)
    assert above.numel() * 8 + elev.numel() * 8 < 0.4e9
    grid = vol.counters.view(vol.shape)
    per_type = [int(above[t].sum().item()) for t in range(2)]
    assert sum(per_type) == total and min(per_type) > 0
    for t in range(2):
        assert per_type[t] == int(elev[t].sum().item()) + int(outside[t].item())
        assert int(outside[t].item()) >= 0
        for f in (0, 1, 7, 40, 99, 150, 222, 299):
            want = grid[t, f].to(torch.int64).bitwise_and(0xFFFFFFFF).sum(dim=0)
            assert torch.equal(above[t, f], want), (t, f)
    assert int(outside.sum().item()) > 0
    del above, elev, outside, grid
    vol.detach()
    e.close()
    del vol
    torch.cuda.empty_cache()


def test_the_host_level_projection_adds_into_host_arrays_at_an_output_frame():
    """r3d_volume_project_to_host (what ./main --scatter-views calls): pieces of a frame range, cut where the groups are
    cut, add up in the host's views to the projection of the whole range; one view alone; its refusals."""
    from radiative3d_amd import _ffi
    L = _ffi.hip_lib()
    shape = (13, 16, 9, 10)
    nx, ny, nz, nf = shape
    desc = grid_desc(shape)
    grid = random_grid(shape, np.random.default_rng(3), 0.3)
    g = _dev(grid)
    n_range, group = 5, 4
    rb = range_bins_numpy(desc, (-20.0, 20.0), 2.5, n_range)
    n_out = n_out_frames(0, nf, group)
    wa, we, wo = project_numpy(grid, 0, nf, group, rb, n_range)
    above = np.zeros((2, n_out, ny, nx), dtype=np.uint64)
    elev = np.zeros((2, n_out, nz, n_range), dtype=np.uint64)
    outside = np.zeros(2, dtype=np.uint64)

    def call(f0, f1, out0, a=above, e=elev, o=outside, m=rb, total=n_out, grp=group):
        p = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        return L.r3d_volume_project_to_host(0, g.data_ptr(), C.byref(desc), f0, f1, grp, p(m), n_range, out0, total, p(a), p(e), p(o))

    for f0, f1 in ((0, 6), (6, 8), (8, 10)):          # an owner's cut inside output frame 1: a head piece, then the rest
        assert call(f0, f1, f0 // group) == 0, L.r3d_last_error()
    assert (above == wa).all() and (elev == we).all() and (outside == wo).all()
    only_above = np.zeros_like(above)
    assert call(0, nf, 0, a=only_above, e=None, o=None, m=None) == 0 and (only_above == wa).all()
    only_elev = np.zeros_like(elev)
    assert call(0, nf, 0, a=None, e=only_elev, o=None) == 0 and (only_elev == we).all()
    assert call(4, 4, 0) == 0                                                       # an empty range: nothing happens
    for kw, match in ((dict(a=None, e=None), "neither view"), (dict(m=None), "column map"), (dict(grp=0), "frame range or group"),
                      (dict(f0=0, f1=11), "frame range or group"), (dict(out0=2), "do not fit")):
        args = dict(f0=0, f1=nf, out0=0)
        args.update(kw)
        assert call(**args) != 0 and match in L.r3d_last_error().decode(), kw
    assert (above == wa).all() and (elev == we).all() and (outside == wo).all()     # (refusals and the empty range left them)
