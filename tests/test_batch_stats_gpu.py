"""Per-bin standard errors from id-partitioned batches on the GPU: the moments kernel alone (r3d_batch_moments),
the batched run against plain runs of the same ids and against the oracle batch by batch, its refusals, the event
grid under it, and ./main --error-batches end to end."""
import subprocess

import numpy as np
import pytest
import torch

from batch_cases import check_se, count_families, families, sum_in_order
from cli_support import main_exe
from octave_text import read_octave
from oracle import oracle_ffi as O
from oracle.check import assert_aggregates_equal
from radiative3d_amd import Engine, _ffi, batch_moments
from tests.configs import halfspace
from tests.test_gpu_parity import energies_agree

pytestmark = pytest.mark.gpu


# ---- the kernel alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 16, 64])
def test_moments_kernel_meets_the_bound_on_every_family(B):
    rng = np.random.default_rng(3000 + B)
    n = 65                                                       # one entry past a wave
    fam, cfam = families(B, n, rng), count_families(B, n, rng)
    cnames = list(cfam)
    for k, (name, x) in enumerate(fam.items()):
        c = cfam[cnames[k % len(cnames)]]
        bx, bc = torch.from_numpy(x).cuda(), torch.from_numpy(c.view(np.int64)).cuda()
        keep_x, keep_c = bx.clone(), bc.clone()
        energy, counts, _, ese, cse = batch_moments(bx, bc)
        again = batch_moments(bx, bc)
        torch.cuda.synchronize()
        assert torch.equal(bx, keep_x) and torch.equal(bc, keep_c)                       # the blocks are only read
        for a, b in zip((energy, counts, ese, cse), (again[0], again[1], again[3], again[4])):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), name            # the same bits every run
        assert (energy.cpu().numpy() == sum_in_order(x)).all(), name
        assert (counts.cpu().numpy().view(np.uint64) == c.sum(axis=0, dtype=np.uint64)).all(), name
        worst = check_se(x, ese.cpu().numpy(), f"{name}, B = {B}")
        check_se(c, cse.cpu().numpy(), f"counts {cnames[k % len(cnames)]}, B = {B}")
        print(f"B = {B:2d} {name:12s} worst error / bound = {worst:.3f}")
        if name in ("all_equal", "all_zero"):
            assert (ese == 0).all(), name


@pytest.mark.parametrize("n", [1, 63, 64, 65, 40961])
def test_moments_kernel_at_ragged_lengths_accumulates_totals_and_sums_scalars(n):
    B = 16
    rng = np.random.default_rng(n)
    x, c = rng.lognormal(0, 3, (B, n)), rng.poisson(9.0, (B, n)).astype(np.int64)
    s = rng.integers(0, 1 << 40, (B, _ffi.R3D_N_SCALARS)).astype(np.int64)
    energy0, counts0 = rng.standard_normal(n), rng.integers(0, 100, n).astype(np.int64)
    # guard entries behind every output: a kernel that ran past `n` would show
    def guarded(a, fill):
        t = torch.full((n + 64,), fill, dtype=torch.from_numpy(a).dtype, device="cuda")
        t[:n] = torch.from_numpy(a).cuda()
        return t
    ge, gc = guarded(energy0, -7.0), guarded(counts0, -7)
    energy, counts, scalars, ese, cse = batch_moments(torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda(),
                                                      torch.from_numpy(s).cuda(), energy=ge[:n], counts=gc[:n])
    torch.cuda.synchronize()
    assert (ge[n:] == -7.0).all() and (gc[n:] == -7).all()
    assert (energy.cpu().numpy() == energy0 + sum_in_order(x)).all()                   # += : the result accumulates
    assert (counts.cpu().numpy() == counts0 + c.sum(0)).all()
    assert (scalars.cpu().numpy() == s.sum(0)).all()
    pick = np.unique(np.concatenate([np.arange(min(n, 70)), np.arange(max(n - 70, 0), n)]))
    check_se(x[:, pick], ese.cpu().numpy()[pick], f"len {n}")
    check_se(c[:, pick].astype(np.uint64), cse.cpu().numpy()[pick], f"counts, len {n}")
    want = np.sqrt(((x - x.mean(0)) ** 2).sum(0) * B / (B - 1))
    assert np.allclose(ese.cpu().numpy(), want, rtol=1e-9, atol=0)                      # (every entry, loosely, against numpy)


# ---- the batched run ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(models):
    cache = {}

    def get(name, extra=()):
        if (name, tuple(extra)) not in cache:
            cache[(name, tuple(extra))] = Engine(models(name, 4, extra))
        return cache[(name, tuple(extra))]
    return get


@pytest.mark.parametrize("name,n", [("halfspace", 50000), ("crustpinch", 20000), ("lopnor", 20000), ("sphere", 3000)])
def test_batched_run_equals_its_batches_the_plain_run_and_the_oracle(engines, name, n):
    B, seed = 10, 0x5EED
    e = engines(name)
    model = e.model
    res, ese, cse, be, bc = e.run_batched(n, B, keep_batches=True)
    assert be.shape == (B,) + res.energy.shape and bc.shape == (B,) + res.counts.shape
    assert res.n_lost + res.n_timeout + res.n_invalid == n
    per = n // B
    # (a) every kept block against a run of its own id range: integers exactly, energies to the engine-vs-engine rule
    scalars = np.zeros(_ffi.R3D_N_SCALARS, dtype=np.uint64)
    alones = []
    for j in range(B):
        alone = e.run(per, first_id=j * per, seed=seed)
        alones.append(alone)
        assert (bc[j] == alone.counts).all(), (name, j)
        assert energies_agree(alone.energy, be[j]), (name, j)
        scalars += alone.scalars()
    assert (res.scalars() == scalars).all()
    # (b) the totals against one plain run of all the ids
    plain = e.run(n, seed=seed)
    assert (res.counts == plain.counts).all() and (res.scalars() == plain.scalars()).all()
    assert energies_agree(plain.energy, res.energy), name
    assert (res.energy == sum_in_order(be)).all()
    # (c) the standard errors against the exact reference on the kept blocks, at the derived bound (every entry with
    #     a catch in it, and a stretch of empty ones)
    flat_e, flat_c = be.reshape(B, -1), bc.reshape(B, -1)
    hit = np.flatnonzero(flat_e.any(axis=0))
    assert len(hit) > 100, (name, len(hit))
    pick = np.concatenate([hit[:: max(1, len(hit) // 1500)], np.arange(0, flat_e.shape[1], max(1, flat_e.shape[1] // 200))])
    worst = check_se(flat_e[:, pick], ese.reshape(-1)[pick], f"{name} energy_se")
    hit_c = np.flatnonzero(flat_c.any(axis=0))
    pick_c = np.concatenate([hit_c[:: max(1, len(hit_c) // 1500)], np.arange(0, flat_c.shape[1], max(1, flat_c.shape[1] // 200))])
    check_se(flat_c[:, pick_c], cse.reshape(-1)[pick_c], f"{name} counts_se")
    print(f"{name}: energy_se worst error / bound = {worst:.3f} over {len(pick)} entries")
    want = np.sqrt(((flat_e - flat_e.mean(0)) ** 2).sum(0) * B / (B - 1))
    assert np.allclose(ese.reshape(-1), want, rtol=1e-9, atol=1e-300)
    assert (ese.reshape(-1)[~flat_e.any(axis=0)] == 0).all()
    # (d) the oracle, batch by batch: every block's aggregates as the parity tests hold them, and counts_se from
    #     the ORACLE's blocks
    oc = np.zeros_like(bc)
    for j in range(B):
        want_j = O.run(model, per, j * per, seed)
        got_j = alones[j]                                        # (the batch's scalars; for its bins, block j itself)
        got_j.energy[:], got_j.counts[:] = be[j], bc[j]
        assert_aggregates_equal(got_j, want_j, f"{name} batch {j}")
        oc[j] = want_j.counts
    assert (res.counts == oc.sum(axis=0, dtype=np.uint64)).all()
    check_se(oc.reshape(B, -1)[:, pick_c], cse.reshape(-1)[pick_c], f"{name} counts_se against the oracle's batches")
    # the host-result entry point (r3d_run_batched, engine-owned scratch) gives the same numbers
    res2, ese2, cse2 = e.run_batched(n, B)
    assert (res2.counts == res.counts).all() and (res2.scalars() == res.scalars()).all()
    assert energies_agree(res.energy, res2.energy) and np.allclose(ese2, ese, rtol=1e-9, atol=1e-300)
    assert np.allclose(cse2, cse, rtol=1e-12, atol=0)


def test_batches_that_do_not_divide_the_run_partition_it(engines):
    e = engines("crustpinch")
    n, B, first = 1003, 64, 2 ** 40 + 5
    res, ese, cse, be, bc = e.run_batched(n, B, first_id=first, seed=0xABCDEF, keep_batches=True)
    plain = e.run(n, first_id=first, seed=0xABCDEF)
    assert (res.counts == plain.counts).all() and (res.scalars() == plain.scalars()).all()
    assert energies_agree(plain.energy, res.energy)
    for j in (0, 1, 37, 63):                                     # batch j is the ids [floor(j n / B), floor((j + 1) n / B))
        lo, hi = j * n // B, (j + 1) * n // B
        alone = e.run(hi - lo, first_id=first + lo, seed=0xABCDEF)
        assert (bc[j] == alone.counts).all() and energies_agree(alone.energy, be[j]), j


def test_refusals_leave_the_callers_buffers_alone(engines):
    e = engines("crustpinch")
    L = e._lib
    ne, nc = e.model.new_result().energy.size, e.model.new_result().counts.size
    B = 4
    bufs = dict(energy=torch.full((ne,), 3.5, dtype=torch.float64, device="cuda"),
                counts=torch.full((nc,), 7, dtype=torch.int64, device="cuda"),
                scalars=torch.full((_ffi.R3D_N_SCALARS,), 9, dtype=torch.int64, device="cuda"),
                ese=torch.full((ne,), -1.0, dtype=torch.float64, device="cuda"),
                cse=torch.full((nc,), -1.0, dtype=torch.float64, device="cuda"),
                be=torch.full((B, ne), 2.5, dtype=torch.float64, device="cuda"),
                bc=torch.full((B, nc), 5, dtype=torch.int64, device="cuda"))
    keep = {k: v.clone() for k, v in bufs.items()}

    def refused(n, batches, match):
        rc = L.r3d_run_device_batched(e._e, n, 0, 0x5EED, batches, bufs["energy"].data_ptr(), bufs["counts"].data_ptr(),
                                      bufs["scalars"].data_ptr(), bufs["ese"].data_ptr(), bufs["cse"].data_ptr(),
                                      bufs["be"].data_ptr(), bufs["bc"].data_ptr(), None)
        torch.cuda.synchronize()
        assert rc != 0 and match in L.r3d_last_error().decode(), (rc, L.r3d_last_error().decode())
        assert all(torch.equal(bufs[k], keep[k]) for k in bufs), match
        with pytest.raises(RuntimeError, match=match):
            e.run_batched(n, batches)

    refused(1000, 1, "at least 2 batches")
    refused(1000, 0, "at least 2 batches")
    refused(1000, 65, "at most 64 batches")
    refused(3, 4, "fewer histories")
    # a carry chain that awaits its flush
    from radiative3d_amd.parallel import DeviceResult
    chain = DeviceResult(e.model, "cuda:0")
    e.run_device(500, 0, 0x5EED, *chain.pointers(), carry="carry")
    torch.cuda.synchronize()
    assert e.carry_pending
    refused(1000, 4, "carried over")
    e.run_device(0, 0, 0x5EED, *chain.pointers(), carry="final")
    torch.cuda.synchronize()
    e.set_event_log(capacity=1 << 12)
    refused(1000, 4, "event log")
    e.set_event_log(mask=0, capacity=0)
    e.set_production_finals(0, 1000)
    refused(1000, 4, "production-finals")
    e.set_production_finals(0, 0)
    # ... and with all of that gone the same call goes through, into the same buffers
    rc = L.r3d_run_device_batched(e._e, 1000, 0, 0x5EED, B, bufs["energy"].data_ptr(), bufs["counts"].data_ptr(),
                                  bufs["scalars"].data_ptr(), bufs["ese"].data_ptr(), bufs["cse"].data_ptr(),
                                  bufs["be"].data_ptr(), bufs["bc"].data_ptr(), None)
    assert rc == 0, L.r3d_last_error().decode()
    torch.cuda.synchronize()
    plain = e.run(1000)
    assert (bufs["counts"].cpu().numpy() - 7 == plain.counts.reshape(-1).astype(np.int64)).all()   # added into the 7s
    assert (bufs["bc"].sum(0).cpu().numpy() == plain.counts.reshape(-1).astype(np.int64)).all()     # blocks zeroed first
    assert (bufs["ese"] >= 0).all() and (bufs["cse"] >= 0).all()                                    # written, not added to


def test_batched_run_fills_an_attached_event_grid_like_a_plain_run(models):
    from tests.test_volume_grid import GRID, VIDEO
    e = Engine(models("crustpinch", 4, VIDEO))
    e.set_volume(**GRID)
    n = 8000
    plain = e.run(n)
    want = e.read_volume(reset=True)
    res, _, _ = e.run_batched(n, 16)
    got = e.read_volume(reset=True)
    assert want.sum() > 10000 and (got == want).all()
    assert res.events == plain.events and (res.counts == plain.counts).all()
    res, *_ = e.run_batched(n, 16, keep_batches=True)
    assert (e.read_volume() == want).all() and res.events == plain.events
    e.close()


def test_cli_error_batches_end_to_end(tmp_path):
    args = halfspace(4) + ["--num-phonons=48K", "--seed=77"]
    plain, batched = tmp_path / "plain", tmp_path / "batched"
    plain.mkdir(), batched.mkdir()
    for out, extra in ((plain, []), (batched, ["--error-batches=16"])):
        r = subprocess.run([main_exe()] + args + [f"--output-dir={out}"] + extra, cwd=out, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert ("Batches: 16" in r.stdout) == bool(extra)
    assert not list(plain.glob("*_err.octv"))
    names = sorted(p.name for p in plain.glob("seis_*.octv"))
    assert len(names) == 144
    some_error = 0
    for name in names:
        a, b = read_octave(plain / name), read_octave(batched / name)
        assert (a["CountPS"] == b["CountPS"]).all(), name
        # (the files print 6 digits: the totals agree to summation order, far below the last printed digit --
        #  one unit of it is allowed for a value that rounds the other way)
        ea, eb = np.hstack([a["TraceXYZ"], a["TracePS"]]), np.hstack([b["TraceXYZ"], b["TracePS"]])
        assert np.allclose(ea, eb, rtol=2e-6, atol=0), name
        err = read_octave(batched / name.replace(".octv", "_err.octv"))
        assert err["NumBatches"] == 16
        assert err["TraceXYZ_se"].shape == a["TraceXYZ"].shape and err["CountPS_se"].shape == a["CountPS"].shape
        assert (err["TracePS_se"] >= 0).all() and ((err["CountPS_se"] > 0) <= (a["CountPS"] > 0)).all()
        # the standard error of a total of non-negative batch values cannot exceed the total (one batch holds it all)
        assert (err["TracePS_se"] <= eb[:, 3:5] * (1 + 1e-5) + 1e-300).all(), name
        some_error += int((err["TracePS_se"] > 0).sum())
    assert some_error > 100


# (the options beyond --error-batches / --job-error-batches, the Batches line, the one file beside the seis files)
CLI_KINDS = {"errors": (["--error-batches=4"], "|  Batches: 4 (standard errors from batch means)", None),
             "lapse": (["--error-batches=4", "--lapse-windows", "--lapse-array=48,95"],
                       "|  Batches: 4 (standard errors from batch means)", "lapse.octv"),
             "image": (["--error-batches=4", "--ttimage", "--ttimage-array=48,95", "--ttimage-fit=4,48"],
                       "|  Batches: 4 (standard errors from batch means)", "ttimage.octv"),
             "job": (["--devices=0,0", "--job-error-batches=4"], "|  Batches: 4 over 2 shards", None)}


@pytest.mark.parametrize("kind", list(CLI_KINDS))
def test_cli_every_batched_kind_says_its_line_once_and_writes_its_files_and_no_other(tmp_path, kind):
    """The four kinds of the batched-run stage (host/batch_out.cpp) through ./main: where the Batches line stands, which
    files there are, which receivers and how many batches they name.  An array that starts at neither end of the model
    is the smallest input at which spreading it and taking it back out can go wrong; the values are the business of the
    end-to-end tests of each kind."""
    extra, line, own = CLI_KINDS[kind]
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([main_exe()] + halfspace(3) + ["--num-phonons=20K", "--seed=77", f"--output-dir={out}"] + extra,
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.split("\n")
    at = [i for i, ln in enumerate(lines) if ln.startswith("|  Batches: ")]
    assert len(at) == 1 and lines[at[0]] == line, [lines[i] for i in at]
    assert lines[at[0] + 1].startswith("|  Shards: "), lines[at[0] + 1]
    assert lines.index("@@ __BEGINNING_SIMULATION__") < at[0]
    want = {f"seis_{s:03d}.octv" for s in range(144)} | {f"seis_{s:03d}_err.octv" for s in range(144)} | ({own} if own else set())
    assert {p.name for p in out.iterdir()} == want
    for s in (0, 48, 143):
        assert read_octave(out / f"seis_{s:03d}_err.octv")["NumBatches"] == 4
    if kind == "lapse":
        got = read_octave(out / "lapse.octv")
        assert (got["LapseSeismometers"][:, 0] == np.arange(48, 96)).all() and got["LapseBatches"] == 4
    if kind == "image":
        got = read_octave(out / "ttimage.octv")
        assert (got["TTSeismometers"][:, 0] == np.arange(48, 96)).all() and got["TTBatches"] == 4
        assert got["TTFitRange"].tolist() == [[4, 48]]
