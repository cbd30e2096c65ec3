"""A run to a target standard error, on the GPU: the judge kernel (r3d_batch_precision) bit for bit against numpy on
crafted arrays, the run in rounds (r3d_run_to_precision) against the job it is by definition -- r3d_node_run_batched on as
many shards as rounds were run --, where it stops, its refusals, and ./main --target-error end to end.  halfspace at TOA
degree 4 throughout, on the reproducible build where two runs are held to each other."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from cli_support import main_exe
from octave_text import read_octave
from precision_cases import ALL, P, S, crafted, met, numpy_judge, spec
from radiative3d_amd import Engine, Node, _ffi, precision_judge
from tests.configs import halfspace
from tests.test_gpu_parity import energies_agree

pytestmark = pytest.mark.gpu

REPRO = os.path.join(_ffi.LIBDIR, "libr3d_hip_repro.so")
SEED = 0x5EED
REL, MIN_COUNT = 0.25, 7
TINY = float(np.finfo(np.float64).tiny)                          # the smallest positive normal double: never reached
M, B = 6000, 4                                                   # a round of the run tests, and its batches
# the stopping test's criterion, fixed here; that a REL of the grid below stops a run of these rounds after the first and
# by the fourth was checked on the host oracle's batches of the same ids when the test was written
STOP_MIN_COUNT, STOP_COVERAGE, STOP_GRID = 3, 0.75, np.logspace(-1.0, 0.5, 61)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the judge alone -----------------------------------------------------------------------------------------------------
def on_device(T, se, counts):
    return (torch.from_numpy(T).cuda(), torch.from_numpy(se).cuda(), torch.from_numpy(counts.view(np.int64)).cuda())


def guarded(A, extra=2):
    """The judge's four outputs with `extra` rows behind the selected receivers', all filled with -7."""
    return (torch.full((A + extra, 3), -7, dtype=torch.int64, device="cuda"),
            torch.full((A + extra,), -7.0, dtype=torch.float64, device="cuda"),
            torch.full((3 + extra,), -7, dtype=torch.int64, device="cuda"),
            torch.full((1 + extra,), -7.0, dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("n_seis,n_bins,first,last,b0,b1,mask", [
    (3, 70, 0, 2, 0, 70, P | S),          # 350 entries a receiver: more than one wave, not a multiple of 64
    (3, 70, 0, 2, 0, 70, ALL),
    (3, 70, 1, 1, 0, 70, ALL),            # a receiver sub-range
    (3, 70, 1, 2, 13, 66, 1 | 4 | 16),    # a bin sub-range that starts inside a wave's stretch
    (3, 1, 0, 2, 0, 1, ALL),              # one bin: five entries a receiver
    (3, 1, 2, 2, 0, 1, P),
    (2, 700, 0, 1, 0, 700, ALL),          # 3500 entries: every work-item of the workgroup loops
])
def test_judge_equals_numpy_bit_for_bit_and_writes_only_its_rows(n_seis, n_bins, first, last, b0, b1, mask):
    T, se, counts = crafted(n_seis, n_bins, REL, MIN_COUNT, 40 + n_bins + mask)
    want = numpy_judge(T, se, counts, first, last, b0, b1, mask, MIN_COUNT, REL)
    d = on_device(T, se, counts)
    keep = [t.clone() for t in d]
    A = last - first + 1
    out = guarded(A)
    rows, worst_rows, totals, worst = precision_judge(*d, first, last, bins=(b0, b1), mask=mask, min_count=MIN_COUNT, rel=REL,
                                                      outputs=out)
    again = precision_judge(*d, first, last, bins=(b0, b1), mask=mask, min_count=MIN_COUNT, rel=REL)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(d, keep))                                # the inputs are only read
    assert (rows[:A].cpu().numpy().view(np.uint64) == want[0]).all(), (rows[:A], want[0])
    assert (bits(worst_rows[:A].cpu().numpy()) == bits(want[1])).all()
    assert (totals[:3].cpu().numpy().view(np.uint64) == want[2]).all()
    assert bits(worst[:1].cpu().numpy())[0] == bits(want[3])[0]
    assert (rows[A:] == -7).all() and (worst_rows[A:] == -7).all() and (totals[3:] == -7).all() and (worst[1:] == -7).all()
    for a, b in zip((rows[:A], worst_rows[:A], totals[:3], worst[:1]), again):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))                      # the same bits on every run
    if n_bins > 1 and mask == ALL:
        assert want[2][0] > want[2][1] > 0 and want[2][2] > 0


def test_judge_refusals_enqueue_nothing():
    T, se, counts = crafted(3, 70, REL, MIN_COUNT, 5)
    d = on_device(T, se, counts)
    out = guarded(3)
    L = _ffi.hip_lib()
    good = dict(first=0, last=2, b0=0, b1=70, mask=P | S, min_count=1, rel=0.1, coverage=0.9)
    ptrs = [t.data_ptr() for t in d], [t.data_ptr() for t in out]
    stream = torch.cuda.current_stream().cuda_stream

    def call(sp, ins=None, outs=None):
        return L.r3d_batch_precision(0, *(ins or ptrs[0]), 3, 70, C.byref(sp) if sp is not None else None, *(outs or ptrs[1]), stream)

    for k in range(3):
        assert call(spec(3, 70, **good), ins=[None if i == k else p for i, p in enumerate(ptrs[0])]) != 0
        assert "null argument" in L.r3d_last_error().decode()
    for k in range(4):
        assert call(spec(3, 70, **good), outs=[None if i == k else p for i, p in enumerate(ptrs[1])]) != 0
        assert "null argument" in L.r3d_last_error().decode()
    assert call(None) != 0 and "null precision spec" in L.r3d_last_error().decode()
    for change, why in ((dict(first=2, last=1), "first > last"), (dict(last=3), "beyond the seismometers"),
                        (dict(b0=5, b1=5), "empty"), (dict(b0=9, b1=5), "empty"), (dict(b1=71), "beyond the bins"),
                        (dict(mask=0), "mask is 0"), (dict(mask=32), "beyond the fifth"), (dict(rel=0.0), "rel_target"),
                        (dict(rel=-0.5), "rel_target"), (dict(rel=float("inf")), "rel_target"), (dict(rel=float("nan")), "rel_target"),
                        (dict(coverage=0.0), "coverage"), (dict(coverage=1.5), "coverage"), (dict(coverage=float("nan")), "coverage")):
        assert call(spec(3, 70, **{**good, **change})) != 0 and why in L.r3d_last_error().decode(), change
    bad = spec(3, 70, **good)
    bad.size = 8
    assert call(bad) != 0 and "size" in L.r3d_last_error().decode()
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in out)                                              # nothing was enqueued
    assert call(spec(3, 70, **{**good, "coverage": 1.0})) == 0, L.r3d_last_error().decode()
    torch.cuda.synchronize()
    assert (out[0][:3] >= 0).all() and (out[0][3:] == -7).all()


# ---- the run -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(models):
    return models("halfspace", 4)


@pytest.fixture(scope="module")
def engine(model):
    e = Engine(model, reproducible=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def references(model):
    """What the run is by definition: Node(model, [0] * G).run_batched(G m, G B) for G = 1 .. 4, computed once."""
    refs = {}
    for G in range(1, 5):
        node = Node(model, [0] * G, lib=REPRO)
        refs[G] = node.run_batched(G * M, G * B, seed=SEED)
        node.close()
    return refs


def same_as_reference(got, ref, n):
    """A run's (Result, energy_se, counts_se) against the node job's: integers and counts_se to the bit, energies by
    energies_agree, energy_se at the rtol two runs of one job are held to (tests/test_shard_stats_gpu.py)."""
    res, ese, cse = got[:3]
    want, wese, wcse = ref
    assert res.n_lost + res.n_timeout + res.n_invalid == n and res.events["generated"] == n
    assert (res.counts == want.counts).all() and (res.scalars() == want.scalars()).all()
    assert (bits(cse) == bits(wcse)).all()
    assert energies_agree(want.energy, res.energy)
    assert np.allclose(ese, wese, rtol=1e-9, atol=1e-300)
    assert ese.max() > 0 and cse.max() > 0


def judged(ref, model, rel, min_count=STOP_MIN_COUNT, mask=P | S):
    res, ese, _ = ref
    return numpy_judge(res.energy, ese, res.counts, 0, model.n_seismometers - 1, 0, model.n_bins, mask, min_count, rel)


def test_unreachable_target_runs_every_round_and_is_the_three_shard_job(model, engine, references):
    got = engine.run_to_precision(3 * M, B, 3, 0, model.n_seismometers - 1, min_count=STOP_MIN_COUNT, rel=TINY, coverage=1.0,
                                  seed=SEED)
    report = got[3]
    assert report["rounds"] == 3 and not report["met"] and report["histories"] == 3 * M
    assert report["round_histories"].tolist() == [M, 2 * M, 3 * M]
    same_as_reference(got, references[3], 3 * M)
    # every round's tally is the judge's of the job so far: selected and zero depend on integers and T > 0 only; an entry
    # is within the smallest normal double only with se == 0, and `worst` is large
    for g in range(3):
        want = judged(references[g + 1], model, TINY)
        assert report["n_selected"][g] == want[2][0] and report["n_zero"][g] == want[2][2], g
        assert report["n_within"][g] == want[2][1] and report["worst"][g] == pytest.approx(want[3], rel=1e-9), g
    assert report["n_selected"][2] > 10 and report["worst"][2] > 0.1
    assert (report["per_receiver"].sum(0) == [report["n_selected"][2], report["n_within"][2], report["n_zero"][2]]).all()
    assert report["worst_per_receiver"].max() == report["worst"][2]
    # a second call with `result` given adds into it; the se arrays are written
    first_counts, first_generated = got[0].counts.copy(), got[0].events["generated"]
    twice = engine.run_to_precision(3 * M, B, 3, 0, model.n_seismometers - 1, min_count=STOP_MIN_COUNT, rel=TINY, coverage=1.0,
                                    seed=SEED, result=got[0])
    assert twice[0] is got[0] and (got[0].counts == 2 * first_counts).all() and got[0].events["generated"] == 2 * first_generated
    assert (bits(twice[2]) == bits(got[2])).all() and np.allclose(twice[1], got[1], rtol=1e-9, atol=1e-300)


def test_one_round_is_the_batched_run(model, engine, references):
    got = engine.run_to_precision(M, B, 1, 0, model.n_seismometers - 1, rel=TINY, seed=SEED)
    assert got[3]["rounds"] == 1 and not got[3]["met"]
    same_as_reference(got, engine.run_batched(M, B, seed=SEED), M)
    same_as_reference(got, references[1], M)
    # uneven cuts and another first id: m is no multiple of B
    uneven = engine.run_to_precision(2 * 5003, 3, 2, 0, model.n_seismometers - 1, rel=TINY, seed=SEED, first_id=2 ** 40 + 5)
    node = Node(model, [0, 0], lib=REPRO)
    same_as_reference(uneven, node.run_batched(2 * 5003, 6, first_id=2 ** 40 + 5, seed=SEED), 2 * 5003)
    node.close()


def test_the_run_stops_at_the_first_round_that_is_met(model, engine, references):
    def decisions(rel):
        out = []
        for G in range(1, 5):
            lo, hi = judged(references[G], model, rel * (1 - 1e-6)), judged(references[G], model, rel * (1 + 1e-6))
            out.append((met(lo[2][0], lo[2][1], STOP_COVERAGE), met(hi[2][0], hi[2][1], STOP_COVERAGE), lo[2], hi[2]))
        return out

    chosen = None
    for rel in STOP_GRID:
        d = decisions(rel)
        first = next((G for G in range(1, 5) if d[G - 1][0] or d[G - 1][1]), None)
        if first and first > 1 and all(d[G - 1][0] == d[G - 1][1] for G in range(1, first + 1)):
            chosen = (float(rel), first, d)
            break
    assert chosen, "no REL of the grid stops this run after round 1 and by round 4 with a clear decision at every round"
    rel, stop, d = chosen
    print(f"rel = {rel:.5f}: stops after round {stop}; (selected, within, zero) by round {[x[2].tolist() for x in d[:stop]]}")
    got = engine.run_to_precision(4 * M, B, 4, 0, model.n_seismometers - 1, min_count=STOP_MIN_COUNT, rel=rel,
                                  coverage=STOP_COVERAGE, seed=SEED)
    report = got[3]
    assert report["rounds"] == stop and report["met"] and report["histories"] == stop * M
    for g in range(stop):
        lo, hi = d[g][2], d[g][3]
        assert report["n_selected"][g] == lo[0] == hi[0] and report["n_zero"][g] == lo[2], g
        assert lo[1] <= report["n_within"][g] <= hi[1], g
        assert met(report["n_selected"][g], report["n_within"][g], STOP_COVERAGE) == (g == stop - 1), g
    same_as_reference(got, references[stop], stop * M)
    # a target wide enough is met at once: one round, and the result is the one-round job's
    wide = engine.run_to_precision(4 * M, B, 4, 0, model.n_seismometers - 1, min_count=STOP_MIN_COUNT, rel=1e6,
                                   coverage=STOP_COVERAGE, seed=SEED)
    assert wide[3]["rounds"] == 1 and wide[3]["met"] and wide[3]["histories"] == M
    assert wide[3]["n_within"][0] == wide[3]["n_selected"][0] > 0
    same_as_reference(wide, references[1], M)


def test_refusals_run_nothing_and_leave_the_callers_arrays_alone(model, engine):
    from radiative3d_amd.parallel import DeviceResult
    L, h = engine._lib, engine._e
    rng = np.random.default_rng(3)
    res = model.new_result()
    res.energy[:] = rng.lognormal(0, 1, res.energy.shape)
    res.counts[:] = rng.integers(0, 100, res.counts.shape)
    res.n_lost, res.events["generated"] = 5, 77
    ese, cse = np.full(res.energy.shape, -1.0), np.full(res.counts.shape, -1.0)
    keep = res.energy.copy(), res.counts.copy(), res.scalars().copy()
    S_, nb = model.n_seismometers, model.n_bins
    good = dict(first=0, last=S_ - 1, b0=0, b1=nb, mask=P | S, min_count=3, rel=0.5, coverage=0.75)

    def refused(n_max, n_batches, rounds, match, **change):
        before = L.r3d_launch_count(h)
        sp = spec(S_, nb, **{**good, **{k: v for k, v in change.items() if k in good}})
        if "n_bins" in change:
            sp.n_bins = change["n_bins"]
        rep = _ffi.PrecisionReport()
        rep.size = change.get("report_size", C.sizeof(rep))
        rep.rounds = 99
        c = res._as_c()
        rc = L.r3d_run_to_precision(h, n_max, 0, SEED, n_batches, rounds, C.byref(sp), C.byref(c), ese.ctypes.data_as(_ffi._dp),
                                    cse.ctypes.data_as(_ffi._dp), C.byref(rep))
        assert rc != 0 and match in L.r3d_last_error().decode(), (rc, L.r3d_last_error().decode())
        res._from_c(c)
        assert (res.energy == keep[0]).all() and (res.counts == keep[1]).all() and (res.scalars() == keep[2]).all(), match
        assert (ese == -1.0).all() and (cse == -1.0).all() and rep.rounds == 99, match
        assert L.r3d_launch_count(h) == before, match

    refused(4 * M, B, 0, "1 .. 64")
    refused(65 * 100, B, 65, "1 .. 64")
    refused(4 * M + 1, B, 4, "not a multiple")
    refused(4 * 3, B, 4, "fewer histories")                        # m = 3 < B
    refused(4 * M, 1, 4, "at least 2 batches")
    refused(4 * M, 65, 4, "at most 64 batches")
    refused(4 * M, B, 4, "first > last", first=2, last=1)
    refused(4 * M, B, 4, "beyond the seismometers", last=S_)
    refused(4 * M, B, 4, "empty", b0=7, b1=7)
    refused(4 * M, B, 4, "beyond the bins", b1=nb + 1)
    refused(4 * M, B, 4, "mask is 0", mask=0)
    refused(4 * M, B, 4, "beyond the fifth", mask=32)
    refused(4 * M, B, 4, "rel_target", rel=0.0)
    refused(4 * M, B, 4, "rel_target", rel=float("inf"))
    refused(4 * M, B, 4, "coverage", coverage=0.0)
    refused(4 * M, B, 4, "coverage", coverage=1.01)
    refused(4 * M, B, 4, "not the model's", n_bins=nb - 1, b1=nb - 1)
    refused(4 * M, B, 4, "r3d_precision_report.size", report_size=16)
    chain = DeviceResult(model, "cuda:0")                          # a carry chain that awaits its flush
    assert L.r3d_run_device_carry(h, 500, 0, SEED, *chain.pointers(), None, 0) == 0, L.r3d_last_error().decode()
    torch.cuda.synchronize()
    assert L.r3d_engine_carry_pending(h)
    refused(4 * M, B, 4, "carried over")
    assert L.r3d_run_device_carry(h, 0, 0, SEED, *chain.pointers(), None, 1) == 0, L.r3d_last_error().decode()
    torch.cuda.synchronize()
    assert L.r3d_engine_set_event_log(h, _ffi.R3D_RPT_ALL, 1 << 12) == 0
    refused(4 * M, B, 4, "event log")
    assert L.r3d_engine_set_event_log(h, 0, 0) == 0
    assert L.r3d_engine_set_production_finals(h, 0, 1000) == 0
    refused(4 * M, B, 4, "production-finals")
    assert L.r3d_engine_set_production_finals(h, 0, 0) == 0
    with pytest.raises(RuntimeError, match="not a multiple"):
        engine.run_to_precision(4 * M + 1, B, 4, 0, S_ - 1)
    # ... and with all of that gone the same call goes through: added into the result, se written, B launches a round
    before = L.r3d_launch_count(h)
    got = engine.run_to_precision(2 * 1000, B, 2, 0, S_ - 1, rel=TINY, seed=SEED, result=res)
    assert L.r3d_launch_count(h) == before + 2 * B and got[3]["rounds"] == 2
    assert res.events["generated"] == 77 + 2000 and res.n_lost >= 5 and (res.counts >= keep[1]).all()


# ---- ./main --target-error -------------------------------------------------------------------------------------------------
def test_cli_target_error_end_to_end(tmp_path, engine):
    """halfspace(4) has a model of its own here (the options are part of its arguments); the Python call runs the same ids
    on the module's engine, whose model differs by those options only."""
    rel, cov, min_count, rounds = 0.55, STOP_COVERAGE, STOP_MIN_COUNT, 4
    r = subprocess.run([main_exe()] + halfspace(4) + ["--num-phonons=48K", "--seed=77", "--error-batches=4",
                                                       f"--target-error={rel},{cov},{min_count},{rounds}",
                                                       f"--output-dir={tmp_path}", "--mparams-outfile=out_mparams.octv"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    plain = Engine(engine.model)                                   # ./main runs the shipped build
    res, ese, cse, report = plain.run_to_precision(48000, 4, rounds, 0, engine.model.n_seismometers - 1, min_count=min_count,
                                                   rel=rel, coverage=cov, seed=77)
    plain.close()
    G = report["rounds"]
    p = read_octave(tmp_path / "precision.octv")
    assert p["PrecisionRelTarget"] == rel and p["PrecisionCoverage"] == cov and p["PrecisionMinCount"] == min_count
    assert p["PrecisionMaxRounds"] == rounds and p["PrecisionBatchesPerRound"] == 4 and p["PrecisionComponents"] == "PS"
    assert p["PrecisionSeismometers"].tolist() == [[0, engine.model.n_seismometers - 1]]
    assert p["PrecisionBins"].tolist() == [[0, engine.model.n_bins]]
    assert p["NumPhononsCap"] == 48000 and p["RoundHistories"] == 12000
    assert p["RoundsRun"] == G and p["NumPhononsRun"] == report["histories"] == G * 12000 and p["Met"] == int(report["met"])
    assert p["NumBatches"] == G * 4
    # the judge's tables: integers exactly; `worst` is a ratio of energies two runs agree on to rounding, printed at 17 digits
    table = p["PrecisionRounds"]
    assert table.shape == (G, 6) and (table[:, 0] == np.arange(1, G + 1)).all()
    assert (table[:, 1] == report["round_histories"]).all() and (table[:, 2] == report["n_selected"]).all()
    assert (table[:, 3] == report["n_within"]).all() and (table[:, 4] == report["n_zero"]).all()
    assert np.allclose(table[:, 5], report["worst"], rtol=1e-9)
    rows = p["PrecisionReceivers"]
    assert rows.shape == (engine.model.n_seismometers, 5) and (rows[:, 0] == np.arange(engine.model.n_seismometers)).all()
    assert (rows[:, 1:4] == report["per_receiver"]).all()
    assert np.allclose(rows[:, 4], report["worst_per_receiver"], rtol=1e-9)
    for line in [f"|  Round {g + 1}: {(g + 1) * 12000} histories" for g in range(G)]:
        assert line in r.stdout, r.stdout[-3000:]
    assert f"|  Target {'met' if report['met'] else 'NOT met'} after {G} of {rounds} rounds" in r.stdout
    assert f"|  Batches: {G * 4} (4 a round" in r.stdout
    # out_mparams.octv holds the cap, as the parent writes it
    assert read_octave(tmp_path / "out_mparams.octv")["NumPhonons"] == 48000
    # seis_NNN.octv and seis_NNN_err.octv against the Python call's result, at the files' six digits
    names = sorted(f.name for f in tmp_path.glob("seis_[0-9][0-9][0-9].octv"))
    assert len(names) == engine.model.n_seismometers
    some_error = 0
    for s, name in enumerate(names):
        a = read_octave(tmp_path / name)
        assert (a["CountPS"] == res.counts[s]).all(), name
        # six printed digits against the number itself: half a unit of the sixth digit, 5e-6 of a value that begins with 1;
        # and two runs of the shipped build agree to energies_agree's 1e-11 of the bin's energy by type only (a component all
        # but normal to the motion moves in its leading digits)
        printed = np.hstack([a["TraceXYZ"], a["TracePS"]])
        off = np.abs(printed - res.energy[s]) - 5.1e-6 * np.abs(res.energy[s]) - 1e-11 * res.energy[s][:, 3:5].sum(-1, keepdims=True)
        at = np.unravel_index(np.argmax(off), off.shape)
        assert off[at] <= 1e-300, (name, at, printed[at], res.energy[s][at], res.energy[s][at[0]])
        e = read_octave(tmp_path / name.replace(".octv", "_err.octv"))
        assert e["NumBatches"] == G * 4 and e["NumBins"] == engine.model.n_bins
        assert np.allclose(e["CountPS_se"], cse[s], rtol=1.1e-5, atol=0), name
        room = 1e-10 * res.energy[s][:, 3:5].sum(-1, keepdims=True)
        got_se = np.hstack([e["TraceXYZ_se"], e["TracePS_se"]])
        assert (np.abs(got_se - ese[s]) <= 1.1e-5 * np.abs(ese[s]) + room).all(), name
        some_error += int((e["TracePS_se"] > 0).sum())
    # there were errors to compare: every judged entry -- P or S energy of a bin with arrivals, which no two of the G x 4
    # batches share to the bit -- has one
    assert some_error >= report["n_selected"][-1] > 0
