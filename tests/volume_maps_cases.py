"""The scatter-event grid reduced along time (include/r3d.h r3d_volume_time_maps) written down once more in numpy, for
tests/test_volume_maps.py, test_volume_maps_cli.py and test_volume_maps_gpu.py: the four maps by argmax / max / sum
along the frame axis, the merge of two partial states, and the grids the tests use."""
import numpy as np

from volume_views_cases import random_grid  # noqa: F401  (re-exported: the tests take every grid from here)

NEVER = np.uint32(0xFFFFFFFF)

# (nx, ny, nz, frames): ragged rows (the column path); ragged, and a frame count that is no multiple of the eight loads
# in flight; rows of whole quads and more quads than one workgroup takes; one frame
SHAPES = ((7, 5, 3, 4), (13, 16, 9, 17), (64, 64, 16, 12), (8, 4, 2, 1))


def neutral_maps(grid):
    """(first, peak_frame, peak_count, total) of the grid's cell shape in the neutral state."""
    shape = (2,) + grid.shape[2:]
    return (np.full(shape, NEVER, dtype=np.uint32), np.full(shape, NEVER, dtype=np.uint32),
            np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.uint64))


def merge_numpy(a, b):
    """The update rule applied to two partial states (each a 4-tuple of maps)."""
    af, apf, apc, at = a
    bf, bpf, bpc, bt = b
    take = (bpc > apc) | ((bpc == apc) & (bpc > 0) & (bpf < apf))
    return (np.minimum(af, bf), np.where(take, bpf, apf).astype(np.uint32), np.where(take, bpc, apc).astype(np.uint32),
            at + bt)


def time_maps_numpy(grid, f0, f1, min_count, start=None):
    """grid: uint32 [2][frames][nz][ny][nx].  The maps of frames [f0, f1) -- (first, peak_frame, peak_count, total),
    frames absolute -- merged into `start` (a 4-tuple; None: the neutral state).  Nothing is modified in place."""
    assert min_count >= 1 and 0 <= f0 <= f1 <= grid.shape[1]
    maps = neutral_maps(grid)
    if f1 > f0:
        g = grid[:, f0:f1]
        reached = g >= min_count
        first = np.where(reached.any(axis=1), reached.argmax(axis=1) + f0, NEVER).astype(np.uint32)   # (argmax: the first True)
        peak_count = g.max(axis=1)
        peak_frame = np.where(peak_count > 0, g.argmax(axis=1) + f0, NEVER).astype(np.uint32)        # (the first maximum)
        maps = (first, peak_frame, peak_count, g.sum(axis=1, dtype=np.uint64))
    return maps if start is None else merge_numpy(start, maps)


def peak_ties(grid):
    """(cells that hold an event, those of them that reach their peak in more than one frame)."""
    peak = grid.max(axis=1)
    at_peak = ((grid == peak[:, None]) & (peak[:, None] > 0)).sum(axis=1)
    return int((peak > 0).sum()), int((at_peak > 1).sum())


def tie_grid(shape, rng, density):
    """uint32 [2][frames][nz][ny][nx] with about `density` of the cells non-zero, counts 1 .. 3: peaks reached in several
    frames, so that "the earliest frame wins" decides cells.  With more than one frame at least a tenth of the cells
    that hold an event have such a tie, or this raises: a test cannot quietly lose its ties.  (A grid of ONE frame has
    no ties to lose.)"""
    nx, ny, nz, nf = shape
    g = rng.integers(1, 4, size=(2, nf, nz, ny, nx), dtype=np.uint32)
    g[rng.random(g.shape) >= density] = 0
    if nf > 1:
        cells, tied = peak_ties(g)
        assert cells > 0 and 10 * tied >= cells, f"tie_grid{shape}, density {density}: {tied} of {cells} cells tie at their peak"
    return g


def grids_of(shape, seed):
    """The named grids of one shape: sparse, dense and tied."""
    rng = np.random.default_rng(seed)
    return (("sparse", random_grid(shape, rng, 0.03)), ("dense", random_grid(shape, rng, 0.7)),
            ("tied", tie_grid(shape, rng, 0.6)))


def frame_ranges(nf):
    """The full range and an inner one (for a grid of one or two frames the inner one is a single frame or empty)."""
    return ((0, nf), (min(1, nf), max(min(1, nf), nf - 1)))
