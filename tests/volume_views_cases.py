"""The two video views of the scatter-event grid (include/r3d.h r3d_volume_project / r3d_volume_range_bins) written
down once more in numpy, for tests/test_volume_views.py and tests/test_volume_views_gpu.py: the column map with the
header's operations in the header's order, and the projection as a sum over z and an np.add.at by the map."""
import numpy as np

OUT = np.uint32(0xFFFFFFFF)

# (nx, ny, nz, frames): ragged rows, rows of whole quads, a frame of more quads than a workgroup takes at a time
SHAPES = ((7, 5, 3, 4), (13, 16, 9, 10), (64, 64, 16, 12))


def centres(desc):
    nx, ny = int(desc.dims[0]), int(desc.dims[1])
    x = desc.origin[0] + (np.arange(nx, dtype=np.float64) + 0.5) * desc.cell_size[0]
    y = desc.origin[1] + (np.arange(ny, dtype=np.float64) + 0.5) * desc.cell_size[1]
    return x, y


def azimuth_offsets(desc, epicentre, azimuth):
    """wrap180(atan2(dy, dx) in degrees - azimuth) of every column centre, [ny][nx]."""
    x, y = centres(desc)
    dx = (x - epicentre[0])[None, :] + np.zeros((y.size, 1))
    dy = (y - epicentre[1])[:, None] + np.zeros((1, x.size))
    d = np.arctan2(dy, dx) * (180.0 / np.pi) - azimuth
    return d - 360.0 * np.floor((d + 180.0) / 360.0)


def range_bins_numpy(desc, epicentre, dr, n_range, azimuth=0.0, half_width=180.0):
    x, y = centres(desc)
    dx = (x - epicentre[0])[None, :] + np.zeros((y.size, 1))
    dy = (y - epicentre[1])[:, None] + np.zeros((1, x.size))
    rho = np.sqrt(dx * dx + dy * dy)
    ir = np.floor(rho / dr)
    view = ir < n_range
    if not half_width >= 180.0:
        view &= np.abs(azimuth_offsets(desc, epicentre, azimuth)) <= half_width
    return np.where(view, np.where(view, ir, 0).astype(np.uint32), OUT)


def n_out_frames(f0, f1, group):
    return -(-(f1 - f0) // group)


def project_numpy(grid, f0, f1, group, range_bin=None, n_range=0):
    """grid: uint32 [2][frames][nz][ny][nx].  Returns (above, elev, outside) as uint64 arrays (elev / outside None
    without a map)."""
    _, _, nz, ny, nx = grid.shape
    n_out = n_out_frames(f0, f1, group)
    above = np.zeros((2, n_out, ny, nx), dtype=np.uint64)
    elev = outside = None
    if range_bin is not None:
        elev = np.zeros((2, n_out, nz, n_range), dtype=np.uint64)
        outside = np.zeros(2, dtype=np.uint64)
        inside = range_bin < n_range
    for t in range(2):
        for F in range(n_out):
            block = grid[t, f0 + F * group:min(f0 + (F + 1) * group, f1)].astype(np.uint64).sum(axis=0)   # [nz][ny][nx]
            above[t, F] = block.sum(axis=0)
            if range_bin is not None:
                for iz in range(nz):
                    np.add.at(elev[t, F, iz], range_bin[inside], block[iz][inside])
                outside[t] += block[:, ~inside].sum(dtype=np.uint64)
    return above, elev, outside


def random_grid(shape, rng, density):
    """uint32 [2][frames][nz][ny][nx] with about `density` of the cells non-zero, a few of them large."""
    nx, ny, nz, nf = shape
    g = rng.integers(1, 50, size=(2, nf, nz, ny, nx), dtype=np.uint32)
    g[rng.random(g.shape) >= density] = 0
    big = rng.random(g.shape) < density * 0.01
    g[big] = rng.integers(1 << 20, 1 << 32, size=int(big.sum()), dtype=np.uint64).astype(np.uint32)
    return g


def grid_desc(shape, origin=(-31.0, 12.5, -40.0), cell=(3.0, 2.0, 5.0), frame_dt=1.5):
    from radiative3d_amd.model import volume_desc
    nx, ny, nz, nf = shape
    return volume_desc(origin, cell, (nx, ny, nz), nf, frame_dt)
