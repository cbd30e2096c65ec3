"""A run to a target standard error, the parts that need no GPU: the criterion's arithmetic (radiative3d_amd/precision/
r3d_precision.h, compiled here by the host compiler) against numpy with `==`, the id cuts of a run in rounds against
r3d_node_run_batched's definition in pure integers, the C layout of the two new structs, the refusals the C-ABI decides
on its arguments alone, and ./main --target-error: its help, its refusals, the numbers of its output stage and
precision.octv through the one reader."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cli_support import main_exe
from octave_text import read_octave
from precision_cases import ALL, P, S, build_host_precision, crafted, host_judge, met, numpy_judge, spec
from radiative3d_amd import Model, _ffi
from tests.configs import halfspace

REPO = _ffi.REPO
INCLUDE = os.path.join(REPO, "include")
REL, MIN_COUNT = 0.25, 7


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host_precision(tmp_path_factory.mktemp("precision"))


def same(got, want):
    rows, worst_rows, totals, worst = got
    assert (rows == want[0]).all(), (rows, want[0])
    assert (np.asarray(worst_rows).view(np.uint64) == np.asarray(want[1]).view(np.uint64)).all()
    assert (totals == want[2]).all()
    assert np.float64(worst).view(np.uint64) == np.float64(want[3]).view(np.uint64)


# ---- the header's arithmetic ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, P | S, ALL])
def test_criterion_equals_numpy_for_every_mask_on_every_edge(host, mask):
    n_seis, n_bins = 4, 70
    T, se, counts = crafted(n_seis, n_bins, REL, MIN_COUNT, 100 + mask)
    want = numpy_judge(T, se, counts, 0, n_seis - 1, 0, n_bins, mask, MIN_COUNT, REL)
    same(host_judge(host, T, se, counts, spec(n_seis, n_bins, 0, n_seis - 1, 0, n_bins, mask, MIN_COUNT, REL)), want)
    # every kind of entry is there, on each side of its edge
    assert want[2][0] > want[2][1] > 0 and want[2][2] > 0 and want[3] > REL


def test_the_planted_edges_land_where_the_criterion_says(host):
    """One bin, (T, se) of its five components: T == 0 -> zero; se == 0 -> within; se == rel * T -> within; one ulp above ->
    selected, not within; far above -> not within and the worst.  With one count fewer nothing is judged."""
    T, se, counts = crafted(2, 3, REL, MIN_COUNT, 1)
    one = spec(2, 3, 0, 0, 0, 1, ALL, MIN_COUNT + 1, REL)
    rows, worst_rows, totals, worst = host_judge(host, T, se, counts, one)
    assert rows.tolist() == [[4, 2, 1]] and totals.tolist() == [4, 2, 1] and worst == 1e9 / 4.0
    for k, want in enumerate(([0, 0, 1], [1, 1, 0], [1, 1, 0], [1, 0, 0], [1, 0, 0])):
        sp = spec(2, 3, 0, 0, 0, 1, 1 << k, MIN_COUNT + 1, REL)
        assert host_judge(host, T, se, counts, sp)[2].tolist() == want, k
    # the bin holds MIN_COUNT + 1 arrivals: equal passes, one more does not, and then nothing is tallied at all
    assert host_judge(host, T, se, counts, spec(2, 3, 0, 0, 0, 1, ALL, MIN_COUNT + 2, REL))[2].tolist() == [0, 0, 0]
    same(host_judge(host, T, se, counts, one), numpy_judge(T, se, counts, 0, 0, 0, 1, ALL, MIN_COUNT + 1, REL))


@pytest.mark.parametrize("first,last,b0,b1", [(0, 0, 0, 70), (3, 3, 0, 70), (1, 2, 0, 70), (0, 3, 0, 1), (0, 3, 69, 70),
                                              (0, 3, 1, 69), (2, 3, 17, 18)])
def test_ranges_take_their_first_and_last_receiver_and_bin(host, first, last, b0, b1):
    T, se, counts = crafted(4, 70, REL, MIN_COUNT, 7)
    want = numpy_judge(T, se, counts, first, last, b0, b1, ALL, MIN_COUNT, REL)
    same(host_judge(host, T, se, counts, spec(4, 70, first, last, b0, b1, ALL, MIN_COUNT, REL)), want)
    # a range one entry shorter at either end counts differently: the ends are inside
    if b1 - b0 > 1:
        inner = numpy_judge(T, se, counts, first, last, b0 + 1, b1 - 1, ALL, MIN_COUNT, REL)
        assert inner[2][0] < want[2][0]


def test_one_bin_and_min_count_zero(host):
    T, se, counts = crafted(3, 1, REL, 0, 9)
    for first, last in ((0, 2), (1, 1)):
        same(host_judge(host, T, se, counts, spec(3, 1, first, last, 0, 1, P | S, 0, REL)),
             numpy_judge(T, se, counts, first, last, 0, 1, P | S, 0, REL))


def test_met_needs_one_selected_entry_and_the_coverage(host):
    for n_selected, n_within, coverage in ((0, 0, 0.5), (0, 0, 1.0), (1, 1, 1.0), (1, 0, 1.0), (10, 9, 0.9), (10, 8, 0.9),
                                           (10, 9, 1.0), (10, 10, 1.0), (3, 1, 1.0 / 3.0), (3, 0, 1e-300), (7, 6, 6.0 / 7.0),
                                           (2 ** 53 + 2, 2 ** 53, 1.0)):
        assert bool(host.met(n_selected, n_within, coverage)) == met(n_selected, n_within, coverage), (n_selected, n_within)
    assert not host.met(0, 0, 0.5) and host.met(10, 9, 0.9) and not host.met(10, 9, 1.0) and host.met(10, 10, 1.0)
    # nothing selected -- every count below min_count -- is not met, whatever the target
    T, se, counts = crafted(2, 5, REL, MIN_COUNT, 3)
    totals = host_judge(host, T, se, counts, spec(2, 5, 0, 1, 0, 5, ALL, 10 ** 9, 1e300, 1e-9))[2]
    assert totals.tolist() == [0, 0, 0] and not host.met(int(totals[0]), int(totals[1]), 1e-9)


def test_spec_refusals(host):
    good = dict(first=0, last=2, b0=0, b1=70, mask=P | S, min_count=1, rel=0.1, coverage=0.9)
    assert host.refusal(C.byref(spec(3, 70, **good)), 3, 70) is None
    for change, why in ((dict(first=2, last=1), "first > last"), (dict(last=3), "beyond the seismometers"),
                        (dict(b0=5, b1=5), "empty"), (dict(b0=6, b1=5), "empty"), (dict(b1=71), "beyond the bins"),
                        (dict(mask=0), "mask is 0"), (dict(mask=32), "beyond the fifth"), (dict(mask=63), "beyond the fifth"),
                        (dict(rel=0.0), "rel_target"), (dict(rel=-1.0), "rel_target"), (dict(rel=float("inf")), "rel_target"),
                        (dict(rel=float("nan")), "rel_target"), (dict(coverage=0.0), "coverage"), (dict(coverage=1.0001), "coverage"),
                        (dict(coverage=float("nan")), "coverage")):
        text = host.refusal(C.byref(spec(3, 70, **{**good, **change})), 3, 70)
        assert text is not None and why in text.decode(), (change, text)
    bad_size = spec(3, 70, **good)
    bad_size.size = 8
    assert b"size" in host.refusal(C.byref(bad_size), 3, 70) and b"null" in host.refusal(None, 3, 70)
    assert host.refusal(C.byref(spec(3, 70, **{**good, "coverage": 1.0})), 3, 70) is None
    assert _ffi.R3D_PRECISION_DEFAULT_MASK == P | S


# ---- the id cuts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,m", [(2, 2), (4, 6000), (4, 6001), (7, 10007), (64, 64), (64, 1000003), (5, 2 ** 40 + 3)])
def test_a_rounds_batches_are_the_whole_jobs_batches_for_every_number_of_rounds(host, B, m):
    """Round g, batch k against batch j = g B + k of r3d_node_run_batched's job of N = G B batches over n = G m ids, for
    every G <= 64: the cut does not depend on G, and the rounds tile the ids."""
    R = 64
    lo, hi = C.c_uint64(), C.c_uint64()
    cuts = {}
    for g in range(R):
        for k in range(B):
            host.round_batch(m, B, g, k, C.byref(lo), C.byref(hi))
            cuts[g, k] = (lo.value, hi.value)
            assert lo.value == g * m + k * m // B and hi.value == g * m + (k + 1) * m // B, (g, k)
        assert cuts[g, 0][0] == g * m and cuts[g, B - 1][1] == (g + 1) * m
        assert all(cuts[g, k][1] == cuts[g, k + 1][0] for k in range(B - 1))
    for G in range(1, R + 1):
        n, N = G * m, G * B
        for g in range(G):
            for k in range(B):
                j = g * B + k
                assert cuts[g, k] == (j * n // N, (j + 1) * n // N), (G, g, k)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_ctypes_mirrors_of_the_two_structs_match_the_c_layout(tmp_path):
    fields = {"r3d_precision_spec": [f for f, _ in _ffi.PrecisionSpec._fields_],
              "r3d_precision_report": [f for f, _ in _ffi.PrecisionReport._fields_]}
    lines = []
    for name, fs in fields.items():
        lines.append(f'printf("%zu", sizeof({name}));')
        lines += [f'printf(" %zu", offsetof({name}, {f}));' for f in fs]
        lines.append('printf("\\n");')
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "r3d.h"\nint main(void) {\n' + "\n".join(lines) +
            '\nprintf("%d %u\\n", R3D_PRECISION_MAX_ROUNDS, R3D_PRECISION_DEFAULT_MASK);\nreturn 0;\n}\n')
    src = tmp_path / "s.c"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(tmp_path / "s"), str(src)])
    got = [[int(x) for x in line.split()] for line in subprocess.check_output([str(tmp_path / "s")]).decode().splitlines()]
    for line, t in zip(got, (_ffi.PrecisionSpec, _ffi.PrecisionReport)):
        assert line == [C.sizeof(t)] + [getattr(t, f).offset for f, _ in t._fields_], t
    assert got[2] == [_ffi.R3D_PRECISION_MAX_ROUNDS, _ffi.R3D_PRECISION_DEFAULT_MASK]


def test_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(INCLUDE, "r3d.h")).read()
    for name, n_args in (("r3d_batch_precision", 12), ("r3d_run_to_precision", 11)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        for lib in (_ffi.hip_lib(), _ffi.hip_lib(reproducible=True)):
            f = getattr(lib, name)
            assert f.restype is C.c_int and len(f.argtypes) == n_args, name
    import radiative3d_amd
    assert callable(radiative3d_amd.precision_judge) and callable(radiative3d_amd.Engine.run_to_precision)
    # an add-on in the sense of DESIGN section 4.4: nothing in csrc/ knows of it, and the judge is a kernel of its own
    csrc = os.path.join(REPO, "radiative3d_amd", "csrc")
    for f in os.listdir(csrc):
        assert "precision" not in open(os.path.join(csrc, f), errors="ignore").read(), f
    text = open(os.path.join(REPO, "radiative3d_amd", "precision", "r3d_precision.hip")).read()
    for kernel in ("precision_rows_kernel", "precision_totals_kernel"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\b", text), kernel
    assert "csrc/" not in "".join(re.findall(r'#include\s+"([^"]+)"', text))


def test_the_judge_and_the_run_refuse_bad_arguments_before_any_device_is_touched():
    import torch
    L = _ffi.hip_lib()
    p = C.c_void_p(4096)       # (never dereferenced: no call below gets as far as a launch)
    err = lambda: L.r3d_last_error().decode()   # noqa: E731
    good = dict(first=0, last=2, b0=0, b1=70, mask=P | S, min_count=1, rel=0.1, coverage=0.9)

    def judge(sp, args=None):
        return L.r3d_batch_precision(0, *(args or (p, p, p)), 3, 70, C.byref(sp) if sp is not None else None, p, p, p, p, None)

    for k in range(3):
        assert judge(spec(3, 70, **good), [None if i == k else p for i in range(3)]) != 0 and "null argument" in err()
    assert L.r3d_batch_precision(0, p, p, p, 3, 70, C.byref(spec(3, 70, **good)), p, None, p, p, None) != 0 and "null argument" in err()
    assert judge(None) != 0 and "null precision spec" in err()
    for change, why in ((dict(first=2, last=1), "first > last"), (dict(last=3), "beyond the seismometers"),
                        (dict(b0=5, b1=5), "empty"), (dict(b1=71), "beyond the bins"), (dict(mask=0), "mask is 0"),
                        (dict(mask=32), "beyond the fifth"), (dict(rel=0.0), "rel_target"), (dict(rel=float("inf")), "rel_target"),
                        (dict(coverage=0.0), "coverage"), (dict(coverage=1.5), "coverage")):
        assert judge(spec(3, 70, **{**good, **change})) != 0 and why in err(), change
        assert err().startswith("r3d_batch_precision: ")
    rep = _ffi.PrecisionReport()
    rep.size = C.sizeof(rep)
    assert L.r3d_run_to_precision(None, 100, 0, 1, 4, 2, C.byref(spec(3, 70, **good)), None, None, None, C.byref(rep)) != 0
    assert "null engine" in err()
    if not torch.cuda.is_available():
        assert judge(spec(3, 70, **good)) != 0 and err() == "r3d_batch_precision: no HIP device (or a bad device index)"


# ---- ./main --target-error ---------------------------------------------------------------------------------------------
OK = ["--num-phonons=48K", "--error-batches=4"]


def test_target_error_option_parses_with_its_defaults_and_is_off_otherwise():
    assert Model(halfspace(3)).precision_request is None
    assert Model(halfspace(3) + ["--error-batches=4"]).precision_request is None
    n = Model(halfspace(3)).n_seismometers
    rq = Model(halfspace(3) + OK + ["--target-error=0.05"]).precision_request
    assert rq == dict(first=0, last=n - 1, mask=P | S, min_count=16, rel=0.05, coverage=0.9, rounds=16)
    rq = Model(halfspace(3) + OK + ["--target-error=0.2,1,0,3", "--target-array=2,5", "--target-components=ZXS"]).precision_request
    assert rq == dict(first=2, last=5, mask=1 | 4 | 16, min_count=0, rel=0.2, coverage=1.0, rounds=3)
    assert Model(halfspace(3) + OK + ["--target-error=0.2,0.5"]).precision_request["min_count"] == 16


@pytest.mark.parametrize("extra,message", [
    (["--num-phonons=48K", "--target-error=0.1"], "--target-error needs --error-batches=B"),
    (["--num-phonons=48K", "--job-error-batches=8", "--target-error=0.1"], "--target-error cannot be combined with --job-error-batches"),
    (OK + ["--target-error=0.1", "--lapse-windows"], "--target-error cannot be combined with --lapse-windows"),
    (OK + ["--target-error=0.1", "--ttimage"], "--target-error cannot be combined with --ttimage"),
    (OK + ["--target-error=0.1", "--reports=INV"], "--target-error cannot be combined with --reports"),
    (OK + ["--target-error=0.1", "--gpus=2"], "--target-error runs on one device: --gpus / --devices name 2 shards"),
    (OK + ["--target-error=0.1", "--devices=0,0,0"], "--target-error runs on one device: --gpus / --devices name 3 shards"),
    (OK + ["--target-array=0,1"], "--target-array needs --target-error"),
    (OK + ["--target-components=PS"], "--target-components needs --target-error"),
    (OK + ["--target-error=0.1,0.9,16,7"], "--num-phonons (48000), the cap, must be a multiple of ROUNDS (7)"),
    (["--num-phonons=100", "--error-batches=4", "--target-error=0.1,0.9,16,50"], "a round of --num-phonons / ROUNDS = 2 histories is fewer"),
    (OK + ["--target-error=0"], "REL, the relative standard error aimed at, must be finite and > 0"),
    (OK + ["--target-error=-0.1"], "REL, the relative standard error aimed at"),
    (OK + ["--target-error=inf"], "REL, the relative standard error aimed at"),
    (OK + ["--target-error=0.1,0"], "COVERAGE, the share of the judged entries"),
    (OK + ["--target-error=0.1,1.5"], "COVERAGE, the share of the judged entries"),
    (OK + ["--target-error=0.1,0.9,-1"], "MINCOUNT, the arrivals a bin needs"),
    (OK + ["--target-error=0.1,0.9,16,0"], "ROUNDS must be 1 .. 64 (got 0)"),
    (OK + ["--target-error=0.1,0.9,16,65"], "ROUNDS must be 1 .. 64 (got 65)"),
    (OK + ["--target-error="], "Required value not provided"),
    (OK + ["--target-error=tight"], "cannot interpret 'tight'"),
    (OK + ["--target-error=0.1", "--target-array=3,2"], "--target-array=FIRST,LAST: seismometer indices with 0 <= FIRST <= LAST"),
    (OK + ["--target-error=0.1", "--target-components=PQ"], "--target-components=LETTERS: letters of XYZPS"),
    (OK + ["--target-error=0.1", "--target-components="], "Required value not provided"),
])
def test_target_error_option_refuses_bad_values_and_combinations(extra, message):
    with pytest.raises(RuntimeError, match=re.escape(message)):
        Model(halfspace(3) + extra)


def test_target_array_beyond_the_models_receivers_is_refused_with_the_model_in_hand():
    m = Model(halfspace(3) + OK + ["--target-error=0.1", "--target-array=0,100000"])
    with pytest.raises(RuntimeError, match=re.escape("--target-array=0,100000: the model has the seismometers 0 .. ")):
        m.precision_request


def test_cli_lists_the_options_refuses_in_its_style_and_reaches_the_engine(tmp_path):
    text = subprocess.run([main_exe(), "--help"], capture_output=True, text=True, timeout=60).stdout
    for option in ("--target-error=REL[,COVERAGE[,MINCOUNT[,ROUNDS]]]", "--target-array=FIRST,LAST", "--target-components=LETTERS"):
        assert option in text, option
    assert "defaults, not measurements" in text and "NumPhononsRun" in text and "out_mparams.octv holds the cap" in text

    def run(extra):
        return subprocess.run([main_exe()] + halfspace(3) + [f"--output-dir={tmp_path}"] + extra, cwd=tmp_path, capture_output=True,
                              text=True, timeout=300)

    for extra, message in ((["--num-phonons=48K", "--target-error=0.1"], "--target-error needs --error-batches=B"),
                           (OK + ["--target-error=0.1", "--devices=0,0"], "--target-error runs on one device"),
                           (OK + ["--target-error=0.1", "--ttimage"], "--target-error cannot be combined with --ttimage"),
                           (OK + ["--target-components=P"], "--target-components needs --target-error"),
                           (OK + ["--target-error=0.1,0.9,16,7"], "must be a multiple of ROUNDS (7)")):
        r = run(extra)
        assert r.returncode == 1 and "Error processing command-line options" in r.stdout and message in r.stdout, r.stdout[-2000:]
    r = run(OK + ["--target-error=0.1", "--target-array=0,100000"])      # (needs the model: refused before any device)
    assert r.returncode == 1 and "--target-array=0,100000: the model has the seismometers" in r.stdout, r.stdout[-2000:]
    assert not list(tmp_path.glob("seis_*")) and not (tmp_path / "precision.octv").exists()
    # the one-device refusal of --error-batches keeps its text
    r = run(OK + ["--devices=0,0"])
    assert r.returncode == 1 and "--error-batches runs on one device" in r.stdout
    import torch
    if not torch.cuda.is_available():                            # a valid command line gets as far as the engine
        r = run(OK + ["--target-error=0.1,0.9,16,4", "--target-array=0,3", "--target-components=PS"])
        assert r.returncode == 1 and "no HIP device" in r.stdout, r.stdout[-2000:]


def test_write_precision_round_trips_through_the_one_reader(tmp_path):
    H = _ffi.host_lib()
    sp = spec(9, 70, 2, 4, 0, 70, 1 | P | S, 16, 0.0625, 0.9)
    rep = _ffi.PrecisionReport()
    rep.size = C.sizeof(rep)
    rep.rounds, rep.met, rep.histories = 3, 1, 36000
    for g in range(3):
        rep.round_histories[g], rep.n_selected[g], rep.n_within[g], rep.n_zero[g] = 12000 * (g + 1), 100 + g, 40 * (g + 1), 7 - g
        rep.worst[g] = 1.0 / (3.0 + g)
    rows = np.arange(9, dtype=np.uint64).reshape(3, 3) + np.uint64(2 ** 40)
    worst_rows = np.array([0.1, 1.0 / 3.0, 5e-324])
    rep.per_receiver, rep.worst_per_receiver = rows.ctypes.data, worst_rows.ctypes.data
    path = tmp_path / "precision.octv"
    assert H.r3dh_write_precision(C.byref(sp), 4, 16, 192000, C.byref(rep), str(path).encode()) == 0, H.r3dh_last_error()
    p = read_octave(path)
    assert list(p) == ["PrecisionRelTarget", "PrecisionCoverage", "PrecisionMinCount", "PrecisionMaxRounds",
                       "PrecisionBatchesPerRound", "PrecisionSeismometers", "PrecisionBins", "PrecisionComponents", "NumPhononsCap",
                       "RoundHistories", "NumPhononsRun", "RoundsRun", "NumBatches", "Met", "PrecisionRounds", "PrecisionReceivers"]
    assert p["PrecisionRelTarget"] == 0.0625 and p["PrecisionCoverage"] == 0.9 and p["PrecisionMinCount"] == 16
    assert p["PrecisionMaxRounds"] == 16 and p["PrecisionBatchesPerRound"] == 4 and p["PrecisionComponents"] == "XPS"
    assert p["PrecisionSeismometers"].tolist() == [[2, 4]] and p["PrecisionBins"].tolist() == [[0, 70]]
    assert p["NumPhononsCap"] == 192000 and p["RoundHistories"] == 12000 and p["NumPhononsRun"] == 36000
    assert p["RoundsRun"] == 3 and p["NumBatches"] == 12 and p["Met"] == 1
    want = np.array([[g + 1, 12000 * (g + 1), 100 + g, 40 * (g + 1), 7 - g, 1.0 / (3.0 + g)] for g in range(3)])
    assert (p["PrecisionRounds"] == want).all()                  # 17 digits: the doubles come back to the bit
    assert (p["PrecisionReceivers"] == np.column_stack([[2, 3, 4], rows.astype(float), worst_rows])).all()
    # without the two arrays the receivers' table is left out; a report of no round is refused
    rep.per_receiver = None
    assert H.r3dh_write_precision(C.byref(sp), 4, 16, 192000, C.byref(rep), str(path).encode()) == 0
    assert "PrecisionReceivers" not in read_octave(path)
    rep.rounds = 0
    assert H.r3dh_write_precision(C.byref(sp), 4, 16, 192000, C.byref(rep), str(path).encode()) != 0
    assert b"rounds" in H.r3dh_last_error()
    assert H.r3dh_write_precision(None, 4, 16, 192000, C.byref(rep), str(path).encode()) != 0


def test_output_stage_numbers_of_batch_plan_equal_numpy(tmp_path):
    from native_build import host_build
    src = r'''
#include "batch_plan.hpp"
extern "C" uint64_t round_histories(uint64_t cap, uint64_t rounds) { return batch_plan::round_histories(cap, rounds); }
extern "C" uint64_t batches_run(uint64_t rounds_run, uint64_t batches) { return batch_plan::batches_run(rounds_run, batches); }
extern "C" void round_table(size_t g, const uint64_t* h, const uint64_t* s, const uint64_t* w, const uint64_t* z, const double* worst,
                            double* out) { batch_plan::round_table(g, h, s, w, z, worst, out); }
extern "C" void receiver_table(size_t first, size_t n, const uint64_t* rows, const double* worst, double* out) {
  batch_plan::receiver_table(first, n, rows, worst, out);
}
'''
    L = C.CDLL(host_build(tmp_path, "libplan.so", src, [os.path.join(REPO, "radiative3d_amd", "host")]))
    L.round_histories.restype = L.batches_run.restype = C.c_uint64
    L.round_histories.argtypes = L.batches_run.argtypes = [C.c_uint64, C.c_uint64]
    for cap, rounds in ((48000, 4), (48000, 7), (0, 3), (64, 64), (10 ** 12, 16), (5, 0)):
        assert L.round_histories(cap, rounds) == (cap // rounds if rounds and cap % rounds == 0 else 0), (cap, rounds)
    assert L.batches_run(3, 4) == 12 and L.batches_run(64, 64) == 4096
    rng = np.random.default_rng(2)
    G, A = 5, 7
    h, s, w, z = (rng.integers(0, 2 ** 50, G).astype(np.uint64) for _ in range(4))
    worst = rng.lognormal(0, 3, G)
    out = np.zeros((G, 6))
    L.round_table.argtypes = [C.c_size_t] + [C.c_void_p] * 6
    L.round_table(G, h.ctypes.data, s.ctypes.data, w.ctypes.data, z.ctypes.data, worst.ctypes.data, out.ctypes.data)
    assert (out == np.column_stack([np.arange(1, G + 1), h.astype(float), s.astype(float), w.astype(float), z.astype(float), worst])).all()
    rows, rworst = rng.integers(0, 2 ** 50, (A, 3)).astype(np.uint64), rng.lognormal(0, 3, A)
    out = np.zeros((A, 5))
    L.receiver_table.argtypes = [C.c_size_t, C.c_size_t] + [C.c_void_p] * 3
    L.receiver_table(11, A, rows.ctypes.data, rworst.ctypes.data, out.ctypes.data)
    assert (out == np.column_stack([np.arange(11, 11 + A), rows.astype(float), rworst])).all()
