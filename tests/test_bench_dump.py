"""bench.py --dump-outputs: what the timed region left its caller, as float64 .npy files (on CPU: a host
result block and a stand-in for the event grid)."""
import importlib.util
import os
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def filled_result(models):
    res = models("crustpinch", deg=2).new_result()
    rng = np.random.default_rng(1)
    res.energy[...] = rng.random(res.energy.shape)
    res.counts[...] = rng.integers(0, 1 << 40, res.counts.shape, dtype=np.uint64)
    res.n_lost, res.events["generated"] = 17, 12345
    return res


def test_result_block_is_written_as_float64(models, tmp_path):
    bench = load_bench()
    res = filled_result(models)
    shapes = bench.dump_outputs(str(tmp_path / "out"), res, None)
    assert sorted(os.listdir(tmp_path / "out")) == ["counts.npy", "energy.npy", "scalars.npy"]
    loaded = {k: np.load(tmp_path / "out" / f"{k}.npy") for k in shapes}
    assert all(a.dtype == np.float64 and list(a.shape) == shapes[k] for k, a in loaded.items())
    assert np.array_equal(loaded["energy"], res.energy)
    assert np.array_equal(loaded["counts"], res.counts.astype(np.float64))
    assert np.array_equal(loaded["scalars"], res.scalars().astype(np.float64))


def test_event_grid_is_a_fixed_sample_of_the_frames_held(models, tmp_path):
    bench = load_bench()
    res = filled_result(models)
    # count[2][8][z y x = 64]: this rank holds frames 2..4 of both wave types
    counters = torch.arange(2 * 8 * 64, dtype=torch.int64).mul_(2654435761).remainder_(1 << 32)
    counters = torch.where(counters > 0x7FFFFFFF, counters - (1 << 32), counters).to(torch.int32)
    runs = [(2 * 64, 5 * 64), (10 * 64, 13 * 64)]
    volume = types.SimpleNamespace(counters=counters, _valid_runs=lambda: runs)
    bench.dump_outputs(str(tmp_path / "a"), res, volume)
    bench.dump_outputs(str(tmp_path / "b"), res, volume)
    index = np.load(tmp_path / "a" / "volume_sample_index.npy")
    sample = np.load(tmp_path / "a" / "volume_sample.npy")
    assert np.array_equal(index, np.load(tmp_path / "b" / "volume_sample_index.npy"))
    assert np.array_equal(sample, np.load(tmp_path / "b" / "volume_sample.npy"))
    # every held counter is drawn (the sample is larger than the frames), none outside them
    held = np.concatenate([np.arange(b, e) for b, e in runs])
    assert np.array_equal(index, held)
    assert np.array_equal(sample, counters.numpy().view(np.uint32)[held].astype(np.float64))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_MAX_BYTES


def test_event_grid_sample_stays_within_the_budget(models, tmp_path):
    bench = load_bench()
    res = filled_result(models)
    counters = torch.zeros(1 << 24, dtype=torch.int32)
    volume = types.SimpleNamespace(counters=counters, _valid_runs=lambda: [(0, counters.numel())])
    shapes = bench.dump_outputs(str(tmp_path / "out"), res, volume)
    assert 0.9 * bench.DUMP_VOLUME_SAMPLES < shapes["volume_sample"][0] <= bench.DUMP_VOLUME_SAMPLES
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")) <= bench.DUMP_MAX_BYTES
