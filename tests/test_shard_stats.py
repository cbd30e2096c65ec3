"""Standard errors for a job sharded over several devices, the parts that need no GPU: the per-entry arithmetic of a
shard's half and of the root's merge (radiative3d_amd/stats/r3d_batch_moments.h, compiled here by the host compiler)
against the exact reference over all N = D * B batches, the two exactness conditions, the --job-error-batches option and
the C-ABI's new names."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from batch_cases import bound, count_families, exact_se, families, sum_in_order
from cli_support import main_exe
from radiative3d_amd import Model, _ffi
from shard_cases import SHARDS, build_host_shard_stats, host_job
from tests.configs import halfspace

REPO = _ffi.REPO
LEN = 40


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host_shard_stats(tmp_path_factory.mktemp("shard_stats"))


def worst_ratio(x, se, N, what):
    """Every entry of se against exact_se over all N rows of x, at bound(N, ...); the worst error / bound."""
    worst = 0.0
    for i in range(x.shape[1]):
        want = exact_se(x[:, i])
        lim = bound(N, x[:, i], want)
        err = abs(float(se[i]) - want)
        assert err <= lim, f"{what}: entry {i}: se {se[i]!r}, exact {want!r}, error {err:.3e} > bound {lim:.3e}"
        if lim > 0:
            worst = max(worst, err / lim)
    return worst


@pytest.mark.parametrize("D,B", SHARDS)
def test_merged_energy_se_meets_the_bound_over_all_the_jobs_batches(host, D, B):
    N = D * B
    rng = np.random.default_rng(5000 + 100 * D + B)
    worst = 0.0
    for name, x in families(N, LEN, rng).items():
        total, se, sums, _ = host_job(host, x, D, B)
        assert (sums == np.stack([sum_in_order(x[g * B:(g + 1) * B]) for g in range(D)])).all(), name   # S_g in batch order
        assert (total == sum_in_order(sums)).all(), name                                          # T in shard order
        ratio = worst_ratio(x, se, N, f"{name}, D = {D}, B = {B}")
        worst = max(worst, ratio)
        if name in ("all_equal", "all_zero"):
            assert (se == 0.0).all(), name
    print(f"D = {D}, B = {B}: worst energy error / bound = {worst:.3f}")


@pytest.mark.parametrize("D,B", SHARDS)
def test_merged_count_se_is_exact_in_the_total_and_meets_the_bound(host, D, B):
    N = D * B
    rng = np.random.default_rng(6000 + 100 * D + B)
    worst = 0.0
    for name, x in count_families(N, LEN, rng).items():
        total, se, sums, _ = host_job(host, x, D, B)
        assert (total == x.sum(axis=0, dtype=np.uint64)).all(), name
        assert (sums == np.stack([x[g * B:(g + 1) * B].sum(axis=0, dtype=np.uint64) for g in range(D)])).all(), name
        worst = max(worst, worst_ratio(x, se, N, f"counts {name}, D = {D}, B = {B}"))
        if name in ("all_equal", "all_zero"):
            assert (se == 0.0).all(), name
    print(f"D = {D}, B = {B}: worst count error / bound = {worst:.3f}")


@pytest.mark.parametrize("B", [2, 3, 16, 64])
def test_one_shard_merged_is_the_one_device_estimator_to_the_bit(host, B):
    rng = np.random.default_rng(7000 + B)
    for name, x in families(B, LEN, rng).items():
        x = np.ascontiguousarray(x)
        total, se, _, _ = host_job(host, x, 1, B)
        t1, se1 = np.empty(LEN), np.empty(LEN)
        host.moments_f64(x.ctypes.data, LEN, B, t1.ctypes.data, se1.ctypes.data)
        assert (total.view(np.uint64) == t1.view(np.uint64)).all() and (se.view(np.uint64) == se1.view(np.uint64)).all(), name
    for name, x in count_families(B, LEN, rng).items():
        x = np.ascontiguousarray(x)
        total, se, _, _ = host_job(host, x, 1, B)
        t1, se1 = np.empty(LEN, dtype=np.uint64), np.empty(LEN)
        host.moments_u64(x.ctypes.data, LEN, B, t1.ctypes.data, se1.ctypes.data)
        assert (total == t1).all() and (se.view(np.uint64) == se1.view(np.uint64)).all(), name


def test_the_split_is_the_textbook_value(host):
    """Batches 1 .. 6 as 3 shards of 2 or 2 shards of 3: T = 21, se = sqrt(6/5 * 17.5) = sqrt(21) either way."""
    x = np.arange(1.0, 7.0).reshape(6, 1)
    for D, B in ((3, 2), (2, 3), (1, 6)):
        total, se, _, _ = host_job(host, x, D, B)
        assert total[0] == 21.0 and se[0] == pytest.approx(21.0 ** 0.5, rel=1e-15), (D, B)


# ---- --job-error-batches ----------------------------------------------------------------------------------------------
def test_job_error_batches_option_parses_and_is_off_by_default():
    assert Model(halfspace(3)).job_error_batches == 0
    assert Model(halfspace(3) + ["--job-error-batches=16"]).job_error_batches == 16
    assert Model(halfspace(3) + ["--job-error-batches=8", "--devices=0,0"]).job_error_batches == 8
    assert Model(halfspace(3) + ["--job-error-batches=256", "--gpus=4"]).job_error_batches == 256   # N itself may pass 64
    m = Model(halfspace(3) + ["--job-error-batches=6", "--devices=0,0,0"])
    assert m.job_error_batches == 6 and m.error_batches == 0


@pytest.mark.parametrize("extra,message", [
    (["--job-error-batches=1"], "at least 2 batches"),
    (["--job-error-batches=0"], "at least 2 batches"),
    (["--job-error-batches=-4"], "at least 2 batches"),
    (["--job-error-batches=many"], "cannot interpret 'many'"),
    (["--job-error-batches="], "Required value not provided"),
    (["--job-error-batches=9", "--gpus=2"], "multiple of the number of shards (got 9 batches over 2 shards)"),
    (["--job-error-batches=8", "--devices=0,0,0"], "multiple of the number of shards"),
    (["--job-error-batches=2", "--gpus=2"], "must be 2 .. 64 (got 2 batches over 2 shards)"),
    (["--job-error-batches=65"], "must be 2 .. 64 (got 65 batches over 1 shard)"),
    (["--job-error-batches=130", "--devices=0,0"], "must be 2 .. 64"),
    (["--job-error-batches=8", "--error-batches=4"], "cannot be combined with --error-batches"),
    (["--error-batches=4", "--job-error-batches=8"], "cannot be combined with --error-batches"),
    (["--job-error-batches=8", "--reports"], "cannot be combined with --reports"),
    (["--job-error-batches=8", "--reports=INV"], "cannot be combined with --reports"),
])
def test_job_error_batches_option_refuses_bad_values_and_combinations(extra, message):
    with pytest.raises(RuntimeError, match=re.escape(message)):
        Model(halfspace(3) + extra)


def test_cli_refuses_in_the_command_line_style_and_lists_the_option(tmp_path):
    for extra, message in ((["--job-error-batches=9", "--devices=0,0"], "multiple of the number of shards"),
                           (["--job-error-batches=8", "--error-batches=4"], "cannot be combined with --error-batches"),
                           (["--job-error-batches=8", "--reports"], "cannot be combined with --reports")):
        r = subprocess.run([main_exe()] + halfspace(3) + ["--num-phonons=1K", f"--output-dir={tmp_path}"] + extra, cwd=tmp_path,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "Error processing command-line options" in r.stdout and message in r.stdout, r.stdout[-2000:]
    assert not list(tmp_path.glob("seis_*"))
    text = subprocess.run([main_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--job-error-batches=N" in text
    # the one-device option's refusal of several shards keeps its text and now names the way out
    r = subprocess.run([main_exe()] + halfspace(3) + ["--num-phonons=1K", "--error-batches=4", "--devices=0,0",
                                                       f"--output-dir={tmp_path}"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "--error-batches runs on one device" in r.stdout and "--job-error-batches=N" in r.stdout


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "r3d.h")).read()
    L, H = _ffi.hip_lib(), _ffi.host_lib()
    for name, n_args in (("r3d_batch_partial", 14), ("r3d_batch_merge", 17), ("r3d_node_run_batched", 8)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == n_args, name
        assert getattr(_ffi.hip_lib(reproducible=True), name)
    assert "r3dh_job_error_batches" in open(os.path.join(REPO, "include", "r3d_host.h")).read()
    assert H.r3dh_job_error_batches.argtypes and H.r3dh_job_error_batches.restype is C.c_uint32
    import radiative3d_amd
    assert callable(radiative3d_amd.batch_partial) and callable(radiative3d_amd.batch_merge)
    assert callable(radiative3d_amd.Node.run_batched)


def test_the_new_code_stays_outside_the_hashed_kernel_sources_and_has_no_atomics():
    csrc = os.path.join(REPO, "radiative3d_amd", "csrc")
    for f in os.listdir(csrc):
        text = open(os.path.join(csrc, f), errors="ignore").read()
        assert "batch_partial" not in text and "batch_merge" not in text and "node_run_batched" not in text, f
    text = open(os.path.join(REPO, "radiative3d_amd", "stats", "r3d_batch_stats.hip")).read()
    for kernel in ("batch_partial_f64_kernel", "batch_partial_u64_kernel", "batch_merge_f64_kernel", "batch_merge_u64_kernel"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\b", text), kernel
    assert "atomic" not in re.sub(r"//[^\n]*", "", text)


def test_device_level_calls_refuse_bad_arguments_before_any_device_is_touched():
    """Every refusal of r3d_batch_partial / r3d_batch_merge is decided on the arguments alone; on a machine without a GPU
    the well-formed call then says that there is no device."""
    import torch
    L = _ffi.hip_lib()
    p = C.c_void_p(4096)       # (never dereferenced: no call below gets as far as a launch)
    err = lambda: L.r3d_last_error().decode()   # noqa: E731
    for B in (0, 1, 65):
        assert L.r3d_batch_partial(0, B, p, 1, p, 1, None, 0, p, p, p, p, None, None) != 0 and "2 .. 64" in err()
        assert L.r3d_batch_merge(0, 2, B, p, p, 1, p, p, 1, None, 0, p, p, None, p, p, None) != 0 and "2 .. 64" in err()
    assert L.r3d_batch_merge(0, 0, 4, p, p, 1, p, p, 1, None, 0, p, p, None, p, p, None) != 0 and "n_shards == 0" in err()
    assert L.r3d_batch_partial(0, 4, None, 1, p, 1, None, 0, p, p, p, p, None, None) != 0 and "null argument" in err()
    assert L.r3d_batch_partial(0, 4, p, 1, p, 1, None, 0, p, None, p, p, None, None) != 0 and "null argument" in err()
    assert L.r3d_batch_partial(0, 4, p, 1, p, 1, p, 19, p, p, p, p, None, None) != 0 and "null argument" in err()
    assert L.r3d_batch_merge(0, 2, 4, None, p, 1, p, p, 1, None, 0, p, p, None, p, p, None) != 0 and "null argument" in err()
    assert L.r3d_batch_merge(0, 2, 4, p, p, 1, p, p, 1, None, 0, p, None, None, p, p, None) != 0 and "null argument" in err()
    assert L.r3d_batch_merge(0, 2, 4, p, None, 1, p, p, 1, None, 0, p, p, None, p, p, None) != 0
    assert "without the shards' squared deviations" in err()
    assert L.r3d_batch_merge(0, 2, 4, p, p, 1, p, None, 1, None, 0, p, p, None, None, p, None) != 0
    assert "without the shards' squared deviations" in err()
    assert L.r3d_node_run_batched(None, 100, 0, 1, 4, None, None, None) != 0 and "null node" in err()
    if not torch.cuda.is_available():
        assert L.r3d_batch_partial(0, 4, p, 1, p, 1, None, 0, p, p, p, p, None, None) != 0
        assert err() == "r3d_batch_partial: no HIP device (or a bad device index)"
        assert L.r3d_batch_merge(0, 2, 4, p, p, 1, p, p, 1, None, 0, p, p, None, p, p, None) != 0
        assert err() == "r3d_batch_merge: no HIP device (or a bad device index)"
