"""Standard errors for a job sharded over several devices, on the GPU: the two device-level kernels (r3d_batch_partial,
r3d_batch_merge) bit for bit against the host build of their arithmetic, the node run (r3d_node_run_batched) on shards
that share a device against one engine's batched run of the same ids, its refusals, and ./main --job-error-batches
end to end.  A node may name a device twice, and the job's batches are cut over the whole id range, so one GPU tests
everything but the copy between two of them (the last test, which waits for a machine with two)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from batch_cases import bound, check_se, count_families, exact_se, families
from cli_support import main_exe
from octave_text import read_octave
from radiative3d_amd import Engine, Node, _ffi, batch_merge, batch_moments, batch_partial
from shard_cases import SHARDS, build_host_shard_stats, host_job
from tests.configs import halfspace
from tests.test_gpu_parity import energies_agree

pytestmark = pytest.mark.gpu

REPRO = os.path.join(_ffi.LIBDIR, "libr3d_hip_repro.so")
LEN = 197                                                        # three waves and a tail of 5
SEED = 0x5EED


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host_shard_stats(tmp_path_factory.mktemp("shard_stats_gpu"))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def worst_ratio(x, se, N, what):
    worst = 0.0
    for i in range(x.shape[1]):
        want = exact_se(x[:, i])
        lim = bound(N, x[:, i], want)
        err = abs(float(se[i]) - want)
        assert err <= lim, f"{what}: entry {i}: se {se[i]!r}, exact {want!r}, error {err:.3e} > bound {lim:.3e}"
        if lim > 0:
            worst = max(worst, err / lim)
    return worst


# ---- the kernels alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B", SHARDS)
def test_partial_and_merge_kernels_equal_the_host_build_and_meet_the_bound(host, D, B):
    N = D * B
    rng = np.random.default_rng(8000 + 100 * D + B)
    fam, cfam = families(N, LEN, rng), count_families(N, LEN, rng)
    cnames = list(cfam)
    worst = 0.0
    for k, (name, x) in enumerate(fam.items()):
        cname = cnames[k % len(cnames)]
        c = cfam[cname]
        s = rng.integers(0, 1 << 40, (N, _ffi.R3D_N_SCALARS)).astype(np.int64)
        dx, dc, ds = torch.from_numpy(x).cuda(), torch.from_numpy(c.view(np.int64)).cuda(), torch.from_numpy(s).cuda()
        keep = dx.clone(), dc.clone()
        states = [batch_partial(dx[g * B:(g + 1) * B], dc[g * B:(g + 1) * B], ds[g * B:(g + 1) * B]) for g in range(D)]
        es, ess, cs, css, ss = (torch.stack([st[i] for st in states]) for i in range(5))
        stacked = [t.clone() for t in (es, ess, cs, css, ss)]
        energy0 = torch.from_numpy(rng.standard_normal(LEN)).cuda()
        energy, counts, scalars, ese, cse = batch_merge(es, ess, cs, css, B, scalars_sum=ss, energy=energy0.clone())
        again = batch_merge(es, ess, cs, css, B, scalars_sum=ss, energy=energy0.clone())
        torch.cuda.synchronize()
        assert torch.equal(dx, keep[0]) and torch.equal(dc, keep[1])                       # the blocks are only read ...
        assert all(torch.equal(a, b) for a, b in zip((es, ess, cs, css, ss), stacked))     # ... and so are the states
        for a, b in zip((energy, counts, scalars, ese, cse), again):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), name             # the same bits every run
        # the host compiler's build of the same header, shard by shard and merged: to the bit
        total, se, sums, sq = host_job(host, x, D, B)
        ctotal, csev, csums, csq = host_job(host, c, D, B)
        assert (bits(es.cpu().numpy()) == bits(sums)).all() and (bits(ess.cpu().numpy()) == bits(sq)).all(), name
        assert (cs.cpu().numpy().view(np.uint64) == csums).all() and (bits(css.cpu().numpy()) == bits(csq)).all(), cname
        assert (bits(energy.cpu().numpy()) == bits(energy0.cpu().numpy() + total)).all(), name     # += : the result accumulates
        assert (bits(ese.cpu().numpy()) == bits(se)).all(), name
        assert (counts.cpu().numpy().view(np.uint64) == ctotal).all() and (bits(cse.cpu().numpy()) == bits(csev)).all(), cname
        assert (scalars.cpu().numpy() == s.sum(0)).all()
        # ... and the exact reference over all N batches, at the bound
        worst = max(worst, worst_ratio(x, ese.cpu().numpy(), N, f"{name}, D = {D}, B = {B}"))
        worst_ratio(c, cse.cpu().numpy(), N, f"counts {cname}, D = {D}, B = {B}")
        if name in ("all_equal", "all_zero"):
            assert (ese == 0).all(), name
        if cname in ("all_equal", "all_zero"):
            assert (cse == 0).all(), cname
        if D == 1:                                                # one shard merged is r3d_batch_moments, to the bit
            e1, c1, s1, ese1, cse1 = batch_moments(dx, dc, ds)
            torch.cuda.synchronize()
            assert (bits(e1.cpu().numpy()) == bits(total)).all() and torch.equal(ese1.view(torch.int64), ese.view(torch.int64))
            assert torch.equal(c1, counts) and torch.equal(cse1.view(torch.int64), cse.view(torch.int64))
            assert torch.equal(s1, scalars)
    print(f"D = {D}, B = {B}: worst energy error / bound = {worst:.3f}")


def test_partial_and_merge_write_nothing_past_their_length_and_refuse_bad_arguments():
    D, B, n = 3, 4, LEN
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.lognormal(0, 3, (D * B, n + 64))).cuda()
    c = torch.from_numpy(rng.poisson(9.0, (D * B, n + 64)).astype(np.int64)).cuda()
    L = _ffi.hip_lib()
    f64 = lambda fill: torch.full((D, n + 64), fill, dtype=torch.float64, device="cuda")   # noqa: E731
    es, ess, css = f64(-7.0), f64(-7.0), f64(-7.0)
    cs = torch.full((D, n + 64), -7, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for g in range(D):           # blocks of n + 64 entries apart would be another layout: a shard's blocks are packed [B][n]
        bx, bc = x[g * B:(g + 1) * B, :n].contiguous(), c[g * B:(g + 1) * B, :n].contiguous()
        assert L.r3d_batch_partial(0, B, bx.data_ptr(), n, bc.data_ptr(), n, None, 0, es[g].data_ptr(), ess[g].data_ptr(),
                                   cs[g].data_ptr(), css[g].data_ptr(), None, stream) == 0, L.r3d_last_error().decode()
    torch.cuda.synchronize()
    for t in (es, ess, css, cs):
        assert (t[:, n:] == -7).all() and (t[:, :n] != -7).all()
    # the merge of packed [D][n] states into guarded outputs
    pes, pess, pcs, pcss = (t[:, :n].contiguous() for t in (es, ess, cs, css))
    out_e = torch.full((n + 64,), -7.0, dtype=torch.float64, device="cuda")
    out_ese, out_cse = out_e.clone(), out_e.clone()
    out_c = torch.full((n + 64,), -7, dtype=torch.int64, device="cuda")
    args = lambda d, b, se=out_ese.data_ptr(), sq=pess.data_ptr(): (   # noqa: E731
        0, d, b, pes.data_ptr(), sq, n, pcs.data_ptr(), pcss.data_ptr(), n, None, 0, out_e.data_ptr(), out_c.data_ptr(), None,
        se, out_cse.data_ptr(), stream)
    for bad, why in ((args(0, B), "n_shards == 0"), (args(D, 1), "2 .. 64"), (args(D, 65), "2 .. 64"),
                     (args(D, B, sq=None), "without the shards' squared deviations")):
        assert L.r3d_batch_merge(*bad) != 0 and why in L.r3d_last_error().decode()
    torch.cuda.synchronize()
    assert (out_e == -7).all() and (out_c == -7).all() and (out_ese == -7).all()           # nothing was enqueued
    assert L.r3d_batch_merge(*args(D, B)) == 0, L.r3d_last_error().decode()
    torch.cuda.synchronize()
    for t in (out_e, out_ese, out_cse, out_c):
        assert (t[n:] == -7).all()
    assert (out_c[:n] == -7 + c[:, :n].sum(0)).all() and (out_ese[:n] >= 0).all()
    # an se array may be left out, and then its squared deviations too
    assert L.r3d_batch_merge(*args(D, B, se=None, sq=None)) == 0, L.r3d_last_error().decode()
    torch.cuda.synchronize()
    assert (out_c[:n] == -7 + 2 * c[:, :n].sum(0)).all()


# ---- the node run ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(models):
    return models("halfspace", 4)


@pytest.fixture(scope="module")
def engine(model):
    e = Engine(model, reproducible=True)
    yield e
    e.close()


def held_against_one_engine(engine, node, n, N, first_id=0):
    """node.run_batched(n, N) against engine.run_batched(n, N, keep_batches=True) of the same ids and seed."""
    one, ese1, cse1, be, bc = engine.run_batched(n, N, first_id=first_id, seed=SEED, keep_batches=True)
    res, ese, cse = node.run_batched(n, N, first_id=first_id, seed=SEED)
    assert res.n_lost + res.n_timeout + res.n_invalid == n
    assert (res.counts == one.counts).all() and (res.scalars() == one.scalars()).all()     # integers: exactly
    assert energies_agree(one.energy, res.energy)                                          # energies: to summation order
    # the node's se against the exact reference on the one engine's kept blocks (the reproducible build makes a batch's
    # block independent of the engine that ran it): every entry with a catch in it, and a stretch of empty ones
    flat_e, flat_c = be.reshape(N, -1), bc.reshape(N, -1)
    hit = np.flatnonzero(flat_e.any(axis=0))
    assert len(hit) > 100, len(hit)
    pick = np.concatenate([hit[:: max(1, len(hit) // 1500)], np.arange(0, flat_e.shape[1], max(1, flat_e.shape[1] // 200))])
    worst = check_se(flat_e[:, pick], ese.reshape(-1)[pick], f"node energy_se, n = {n}, N = {N}")
    hit_c = np.flatnonzero(flat_c.any(axis=0))
    pick_c = np.concatenate([hit_c[:: max(1, len(hit_c) // 1500)], np.arange(0, flat_c.shape[1], max(1, flat_c.shape[1] // 200))])
    worst_c = check_se(flat_c[:, pick_c], cse.reshape(-1)[pick_c], f"node counts_se, n = {n}, N = {N}")
    print(f"n = {n}, N = {N} over {len(node)} shards: energy_se worst error / bound = {worst:.3f}, counts_se {worst_c:.3f}")
    assert (ese.reshape(-1)[~flat_e.any(axis=0)] == 0).all() and (ese >= 0).all() and (cse >= 0).all()
    assert ese.max() > 0 and cse.max() > 0
    return res, ese, cse


def test_node_on_a_shared_device_equals_one_engines_batched_run(model, engine):
    node = Node(model, [0, 0], lib=REPRO)
    res, ese, cse = held_against_one_engine(engine, node, 20000, 8)
    # once more: the integer side has the same bits on every run (a bin's energy is summed by atomics inside a launch,
    # in an order that varies, so the energy blocks themselves agree to rounding only), and *out is ADDED into
    again = node.run_batched(20000, 8, seed=SEED)
    assert (bits(again[2]) == bits(cse)).all() and (again[0].counts == res.counts).all()
    assert energies_agree(res.energy, again[0].energy) and np.allclose(again[1], ese, rtol=1e-9, atol=1e-300)
    twice = node.run_batched(20000, 8, seed=SEED, result=res)[0]
    assert twice is res and (res.counts == 2 * again[0].counts).all() and res.events["generated"] == 40000
    node.close()


def test_node_with_uneven_cuts_and_the_fewest_batches_per_shard(model, engine):
    node = Node(model, [0, 0, 0], lib=REPRO)                     # B = 2; floor(j 10007 / 6) does not divide evenly
    held_against_one_engine(engine, node, 10007, 6, first_id=2 ** 40 + 5)
    node.close()


def test_node_refusals_run_nothing_and_leave_the_callers_arrays_alone(model):
    from radiative3d_amd.parallel import DeviceResult
    node = Node(model, [0, 0], lib=REPRO)
    L = node._lib
    handles = [node.engine(g) for g in range(2)]
    rng = np.random.default_rng(3)
    res = model.new_result()
    res.energy[:] = rng.lognormal(0, 1, res.energy.shape)
    res.counts[:] = rng.integers(0, 100, res.counts.shape)
    res.n_lost, res.events["generated"] = 5, 77
    ese, cse = np.full(res.energy.shape, -1.0), np.full(res.counts.shape, -1.0)
    keep = res.energy.copy(), res.counts.copy(), res.scalars().copy()

    def refused(n, N, match):
        before = [L.r3d_launch_count(h) for h in handles]
        c = res._as_c()
        rc = L.r3d_node_run_batched(node._n, n, 0, SEED, N, C.byref(c), ese.ctypes.data_as(_ffi._dp), cse.ctypes.data_as(_ffi._dp))
        assert rc != 0 and match in L.r3d_last_error().decode(), (rc, L.r3d_last_error().decode())
        res._from_c(c)
        assert (res.energy == keep[0]).all() and (res.counts == keep[1]).all() and (res.scalars() == keep[2]).all(), match
        assert (ese == -1.0).all() and (cse == -1.0).all(), match
        assert [L.r3d_launch_count(h) for h in handles] == before, match
        with pytest.raises(RuntimeError, match=match):
            node.run_batched(n, N, seed=SEED)

    refused(1000, 9, "not a multiple")
    refused(1000, 2, "at least 2 batches per shard")
    refused(1000, 130, "at most 64 batches per shard")
    refused(7, 8, "fewer histories")
    chain = DeviceResult(model, "cuda:0")                        # a carry chain that awaits its flush, on the second shard
    assert L.r3d_run_device_carry(handles[1], 500, 0, SEED, *chain.pointers(), None, 0) == 0, L.r3d_last_error().decode()
    torch.cuda.synchronize()
    assert L.r3d_engine_carry_pending(handles[1])
    refused(1000, 8, "carried over")
    assert L.r3d_run_device_carry(handles[1], 0, 0, SEED, *chain.pointers(), None, 1) == 0, L.r3d_last_error().decode()
    torch.cuda.synchronize()
    assert L.r3d_engine_set_event_log(handles[0], _ffi.R3D_RPT_ALL, 1 << 12) == 0
    refused(1000, 8, "event log")
    assert L.r3d_engine_set_event_log(handles[0], 0, 0) == 0
    assert L.r3d_engine_set_production_finals(handles[1], 0, 1000) == 0
    refused(1000, 8, "production-finals")
    assert L.r3d_engine_set_production_finals(handles[1], 0, 0) == 0
    # ... and with all of that gone the same call goes through: added into the result, se written
    before = [L.r3d_launch_count(h) for h in handles]
    c = res._as_c()
    assert L.r3d_node_run_batched(node._n, 1000, 0, SEED, 8, C.byref(c), ese.ctypes.data_as(_ffi._dp),
                                  cse.ctypes.data_as(_ffi._dp)) == 0, L.r3d_last_error().decode()
    res._from_c(c)
    assert [L.r3d_launch_count(h) for h in handles] == [b + 4 for b in before]
    plain = node.run(1000, seed=SEED)
    assert (res.counts == keep[1] + plain.counts).all() and res.events["generated"] == 77 + 1000 and res.n_lost >= 5
    assert (ese >= 0).all() and (cse >= 0).all()
    node.close()


# ---- ./main --job-error-batches -----------------------------------------------------------------------------------------
def test_cli_job_error_batches_end_to_end(tmp_path):
    args = halfspace(4) + ["--num-phonons=48K", "--seed=77"]
    one, job = tmp_path / "one", tmp_path / "job"
    one.mkdir(), job.mkdir()
    for out, extra, line in ((one, ["--error-batches=8"], "Batches: 8 (standard errors"),
                             (job, ["--job-error-batches=8", "--devices=0,0"], "|  Batches: 8 over 2 shards")):
        r = subprocess.run([main_exe()] + args + [f"--output-dir={out}"] + extra, cwd=out, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert line in r.stdout, r.stdout[-3000:]
    names = sorted(p.name for p in one.glob("seis_[0-9][0-9][0-9].octv"))
    assert len(names) == 144 and names == sorted(p.name for p in job.glob("seis_[0-9][0-9][0-9].octv"))
    some_error = 0
    for name in names:
        a, b = read_octave(one / name), read_octave(job / name)
        assert (a["CountPS"] == b["CountPS"]).all(), name
        # (the files print 6 digits: the totals agree to summation order, far below the last printed digit)
        ea, eb = np.hstack([a["TraceXYZ"], a["TracePS"]]), np.hstack([b["TraceXYZ"], b["TracePS"]])
        assert np.allclose(ea, eb, rtol=2e-6, atol=0), name
        sa, sb = (read_octave(d / name.replace(".octv", "_err.octv")) for d in (one, job))
        assert sa["NumBatches"] == sb["NumBatches"] == 8 and sb["NumBins"] == sa["NumBins"]
        # the same eight batches, their spread taken flat on one device and in two levels over two shards: the integer
        # columns' se from identical integers, the energies' from blocks that agree to 1e-11 of their bin's energy by
        # type (tests/test_gpu_parity.py energies_agree), which moves an se by at most sqrt(8 * 8/7) * 1e-11 of it
        # (and two values that close can still print one unit of the sixth digit apart: 1e-5 of a value that begins with 1)
        assert np.allclose(sa["CountPS_se"], sb["CountPS_se"], rtol=1.1e-5, atol=0), name
        room = 1e-10 * ea[:, 3:5].sum(-1, keepdims=True)
        for key in ("TraceXYZ_se", "TracePS_se"):
            assert sa[key].shape == sb[key].shape and (np.abs(sa[key] - sb[key]) <= 1.1e-5 * np.abs(sa[key]) + room).all(), (name, key)
        assert (sb["TracePS_se"] <= eb[:, 3:5] * (1 + 1e-5) + 1e-300).all(), name
        some_error += int((sb["TracePS_se"] > 0).sum())
    assert some_error > 100


# ---- two devices ------------------------------------------------------------------------------------------------------------
def test_two_devices_give_what_two_shards_on_one_device_give(model):
    """Waits for a machine with two GPUs: the states then travel between devices."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    shared, spread = Node(model, [0, 0], lib=REPRO), Node(model, [0, 1], lib=REPRO)
    a, b = shared.run_batched(20000, 8, seed=SEED), spread.run_batched(20000, 8, seed=SEED)
    assert (a[0].counts == b[0].counts).all() and (a[0].scalars() == b[0].scalars()).all()
    assert (bits(a[0].energy) == bits(b[0].energy)).all()
    assert (bits(a[1]) == bits(b[1])).all() and (bits(a[2]) == bits(b[2])).all()
    shared.close(), spread.close()
