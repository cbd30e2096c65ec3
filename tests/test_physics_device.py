"""The DEVICE build of the per-lane physics against the oracle, case by case.

tests/test_rt_solve.py, tests/test_face_filter.py and tests/test_guide_cells.py hold the hard cases of
radiative3d_amd/csrc/r3d_physics.h -- critical angles, grazing and normal incidence, fluids, edge and vertex starts,
slivers, tangent arcs, long brackets -- in the g++ build of that header, one lane at a time.  The device build of the same
text differs exactly where those tests cannot see: reciprocals and roots are hardware seeds plus Newton steps, hipcc
contracts a * b + c its own way, the votes (`any_lanes`, `all_lanes`) run with some lanes of a wave in and others out, and
two pieces exist under __HIP_DEVICE_COMPILE__ only: the tetra search by four lanes per history (`tet_fast_exit_quad`,
the drain kernel's) and the address-space-1 path of `sample_cdf_guided`.

Here the SAME case tables (tests/emul/physics_cases.h: generate) go through the SAME evaluator functions in a kernel,
one lane per case (tests/emul/physics_device.hip, `make devtest`), and the output tables through the SAME comparator
and the same assertions as the CPU tests, with the project's one tolerance (1e-9, plus what the reference's own
formulation loses: physics_cases.h cmp_rt / cmp_bend).  Every table has 2^18 + 37 cases: the last wave is partial.

CAVEAT.  libr3d_physics_device.so is a sibling compilation of the same text under the same flags, with its own inlining
and schedule.  It is not the code object of the traversal kernels (the STEPFINALS library of tests/test_gpu_parity.py
carries the same caveat): an error of the source, of the compiler's contraction or of the hardware's seeds shows here;
one that only a kernel's own register allocation provokes does not.

Each device test prints the largest deviations from the oracle per mode, next to the host build's (LOG.md records them).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import emul_ffi as E
import native_build
from oracle import oracle_ffi as O
from test_rt_solve import MARGIN, TOL

HERE = os.path.dirname(os.path.abspath(__file__))
N = 2 ** 18 + 37

# family -> (oracle callback, seed of mode 0 in the CPU tests, modes, mode of the flat-face form)
FAMILIES = {"rt": ("r3d_oracle_rt_event", 20261005, range(10), 9), "bend": ("r3d_oracle_bend_event", 20261006, range(5), 4),
            "rot": ("r3d_oracle_transform", 20261007, range(3), None), "tet": ("r3d_oracle_tet_search", 20261004, range(8), None),
            "shell": ("r3d_oracle_shell_search", 20261004, range(7), None)}
TET_LEAST = {m: (0.98 if m == 0 else 0.25) for m in range(8)}          # tests/test_face_filter.py
SHELL_LEAST = {0: 0.99, 1: 0.8, 2: 0.8, 3: 0.5, 4: 0.3, 5: 0.1, 6: 0.99}


# ---- the three steps -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases(family, mode):
    """The family's table for `mode`, with the CPU test's seed; made once and never written to."""
    table = E.cases_generate(family, mode, N, FAMILIES[family][1] + mode)
    table.setflags(write=False)
    return table


@functools.lru_cache(maxsize=None)
def device_lib(repro=False):
    so = os.path.join(HERE, "emul", "libr3d_physics_device_repro.so" if repro else "libr3d_physics_device.so")
    L = C.CDLL(native_build.make("devtest", missing=so))
    dp = C.POINTER(C.c_double)
    L.r3d_devtest_last_error.restype = C.c_char_p
    L.r3d_devtest_eval.restype = C.c_int
    L.r3d_devtest_eval.argtypes = [C.c_int, C.c_int, C.c_int, dp, dp, C.c_uint64]
    L.r3d_devtest_quad.restype = C.c_int
    L.r3d_devtest_quad.argtypes = [C.c_int, dp, dp, C.c_uint64]
    L.r3d_devtest_guided.restype = C.c_int
    L.r3d_devtest_guided.argtypes = [C.c_int, dp, C.c_uint64, C.c_uint32, dp, C.c_uint64, C.POINTER(C.c_uint64), C.c_int]
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def device_rows(family, table, flat_form=False, repro=False):
    L = device_lib(repro)
    table = np.ascontiguousarray(table, dtype=np.float64)
    out = np.zeros((table.shape[0], E.cases_width(family, True)), dtype=np.float64)
    rc = L.r3d_devtest_eval(0, E.CASE_FAMILIES.index(family), 1 if flat_form else 0, _dp(table), _dp(out), table.shape[0])
    assert rc == 0, L.r3d_devtest_last_error().decode()
    return out


def quad_rows(table, repro=False):
    """[case, lane of the quad, search row] of the tetra search by four lanes per history."""
    L = device_lib(repro)
    table = np.ascontiguousarray(table, dtype=np.float64)
    out = np.zeros((table.shape[0], 4, E.cases_width("tet", True)), dtype=np.float64)
    rc = L.r3d_devtest_quad(0, _dp(table), _dp(out), table.shape[0])
    assert rc == 0, L.r3d_devtest_last_error().decode()
    return out


@functools.lru_cache(maxsize=None)
def device_search(mode, repro=False):
    """The single-lane device search of tetra table `mode` (shared by the search, the quad and the repro tests)."""
    out = device_rows("tet", cases("tet", mode), repro=repro)
    out.setflags(write=False)
    return out


EVENT_KEYS = {"rt": ("cases", "outcome_differs", "outcome_differs_outside_margin", "direction_off", "polarisation_off",
                     "transmitted", "s_out", "sh_in"),
              "bend": ("cases", "side_differs", "side_differs_outside_margin", "direction_off", "polarisation_off", "crossed", "s_rays"),
              "rot": ("cases", "direction_off", "polarisation_off"),
              "tet": ("cases", "certified", "face_differs", "length_differs", "reference_has_no_exit", "engine_search_vs_oracle"),
              "shell": ("cases", "certified", "face_differs", "length_differs", "reference_has_no_exit", "engine_search_vs_oracle")}


def compare(family, table, out):
    """The comparator of the CPU tests on an output table: its counters by the CPU tests' names."""
    counters, dev, first = E.cases_compare(family, table, out, TOL, MARGIN, getattr(O.lib(), FAMILIES[family][0]))
    r = dict(zip(EVENT_KEYS[family], counters))
    if family in ("tet", "shell"):
        r.update(dev_over_R=dev[0], first=first)
    else:
        r.update(dev_dir=dev[0], dev_pol=dev[1], first=first)
    return r


def both_builds(family, mode, flat_form):
    """(device, host) comparisons of one table; the report line of section "largest deviations" of LOG.md."""
    table = cases(family, mode)
    dev_out = device_search(mode) if family == "tet" else device_rows(family, table, flat_form)
    d, h = compare(family, table, dev_out), compare(family, table, E.cases_evaluate(family, table, flat_form))
    if family in ("tet", "shell"):
        print(f"\n[physics-device] {family} mode {mode}: length/R device {d['dev_over_R']:.3g} host {h['dev_over_R']:.3g}; "
              f"certified device {d['certified'] / N:.4f} host {h['certified'] / N:.4f}")
    else:
        print(f"\n[physics-device] {family} mode {mode}: direction device {d['dev_dir']:.3g} host {h['dev_dir']:.3g}; "
              f"polarisation device {d['dev_pol']:.3g} host {h['dev_pol']:.3g}")
    return d, h


def test_the_steps_one_by_one_are_the_one_call_entries():
    """generate -> evaluate (host) -> compare through the separate entries gives the counters and deviations of the
    r3d_emul_* entries the CPU tests call, for a table that spans more than one of their blocks."""
    from test_face_filter import run as tet_run, run_shell
    from test_rt_solve import run as rt_run
    n = 40_003
    for family, mode, whole in [("rt", 2, rt_run(2, n, 11)), ("rt", 9, rt_run(9, n, 11)), ("tet", 2, tet_run(2, n, 11)), ("shell", 4, run_shell(4, n, 11))]:
        table = E.cases_generate(family, mode, n, 11)
        counters, dev, first = E.cases_compare(family, table, E.cases_evaluate(family, table, family == "rt" and mode == 9), TOL, MARGIN,
                                               getattr(O.lib(), FAMILIES[family][0]))
        for key, got in zip(EVENT_KEYS[family], counters):
            assert whole[key] == got, (family, mode, key)
        assert whole["dev_dir" if family == "rt" else "dev_over_R"] == dev[0] and whole["first"] == first
        assert whole["cases"] == n


# ---- events, bends, rotations -------------------------------------------------------------------------------------
def assert_rt(r, mode, n, shares=True):
    assert r["cases"] == n
    assert r["outcome_differs_outside_margin"] == 0, (mode, r)
    assert r["outcome_differs"] <= 2, (mode, r)
    assert r["direction_off"] == 0 and r["polarisation_off"] == 0, (mode, r)
    if not shares:
        return
    if mode in (1, 5):
        assert r["transmitted"] == 0
    elif mode != 3:
        assert r["transmitted"] > 0.05 * n
    assert r["s_out"] > 0.15 * n
    if mode != 5:
        assert r["sh_in"] > 0.05 * n


def assert_bend(r, mode, n, shares=True):
    assert r["cases"] == n
    assert r["side_differs_outside_margin"] == 0 and r["side_differs"] <= 2, (mode, r)
    assert r["direction_off"] == 0 and r["polarisation_off"] == 0, (mode, r)
    if shares:
        assert r["s_rays"] > 0.4 * n and 0.05 * n < r["crossed"] <= n, (mode, r)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", FAMILIES["rt"][2])
def test_device_event_is_the_oracles_event(mode):
    """tests/test_rt_solve.py test_event_is_the_oracles_event, the events evaluated on the device."""
    d, h = both_builds("rt", mode, mode == 9)
    assert_rt(h, mode, N)
    assert_rt(d, mode, N)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", FAMILIES["bend"][2])
def test_device_bend_is_the_oracles_bend(mode):
    d, h = both_builds("bend", mode, mode == 4)
    assert_bend(h, mode, N)
    assert_bend(d, mode, N)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", FAMILIES["rot"][2])
def test_device_scatter_rotation_is_the_oracles_transform(mode):
    d, h = both_builds("rot", mode, False)
    for r in (h, d):
        assert r["cases"] == N and r["direction_off"] == 0 and r["polarisation_off"] == 0, (mode, r)


# ---- waves whose lanes disagree ----------------------------------------------------------------------------------
def mixed_waves(a, b):
    """Rows of `a` and `b` interleaved in whole-wave patterns, as `_waves` of tests/test_lean_math.py: all a; all b;
    one b lane among 63 a; alternate lanes.  (The last wave is partial.)"""
    rng = np.random.default_rng(20261019)
    lane, wave = np.arange(N) % 64, np.arange(N) // 64
    one = rng.integers(0, 64, wave[-1] + 1)[wave]
    take_b = np.select([wave % 4 == 0, wave % 4 == 1, wave % 4 == 2], [False, True, lane == one], lane % 2 == 0)
    return np.where(take_b[:, None], b, a), take_b


@pytest.mark.gpu
@pytest.mark.parametrize("family,mode_a,mode_b,flat_form", [
    ("rt", 0, 9, True),      # tilted faces among horizontal ones, through the flat-face form: any_lanes(!flat)
    ("rt", 0, 8, False),     # exactly along the normal among oblique rays: any_lanes(is_zero(w)), the substitute axis
    ("bend", 0, 4, True),    # bend<true>: any_lanes(!flat)
    ("tet", 0, 6, False),    # two_atan: all_lanes(t <= 1/16) with short and long legs in one wave
    ("tet", 0, 7, False)])
def test_device_waves_whose_lanes_vote_differently(family, mode_a, mode_b, flat_form):
    """Each row is held to the oracle exactly as in the unmixed tables: the oracle does not care which form served it."""
    table, take_b = mixed_waves(cases(family, mode_a), cases(family, mode_b))
    assert 0.3 * N < take_b.sum() < 0.45 * N
    out = device_rows(family, table, flat_form)
    d = compare(family, table, out)
    if family == "rt":
        assert_rt(d, (mode_a, mode_b), N, shares=False)
    elif family == "bend":
        assert_bend(d, (mode_a, mode_b), N, shares=False)
    else:
        assert_search(d, (mode_a, mode_b), 0.25)
        # the certificate and the exit are a lane's own: the neighbours change the series two_atan takes, nothing else
        pure = np.where(take_b[:, None], device_search(mode_b), device_search(mode_a))
        assert np.array_equal(out[:, :3].view(np.uint64), pure[:, :3].view(np.uint64))
    print(f"\n[physics-device] mixed waves {family} modes {mode_a}+{mode_b}: " +
          (f"length/R {d['dev_over_R']:.3g}" if family == "tet" else f"direction {d['dev_dir']:.3g} polarisation {d['dev_pol']:.3g}"))


# ---- boundary searches ----------------------------------------------------------------------------------------------
def assert_search(r, mode, least):
    """Wherever the search certifies: the oracle's face and length (tests/test_face_filter.py; its absolute floor of
    100 000 certified cases is for its own sizes)."""
    assert r["cases"] == N and r["certified"] >= least * N, (mode, r)
    assert r["face_differs"] == 0 and r["reference_has_no_exit"] == 0, (mode, r)
    assert r["length_differs"] == 0 and r["dev_over_R"] <= TOL, (mode, r)
    assert r["engine_search_vs_oracle"] == 0, (mode, r)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", FAMILIES["tet"][2])
def test_device_certified_exit_is_the_references_exit(mode):
    d, h = both_builds("tet", mode, False)
    assert_search(h, mode, TET_LEAST[mode])
    assert_search(d, mode, TET_LEAST[mode])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", FAMILIES["shell"][2])
def test_device_certified_shell_exit_is_the_references_exit(mode):
    d, h = both_builds("shell", mode, False)
    assert_search(h, mode, SHELL_LEAST[mode])
    assert_search(d, mode, SHELL_LEAST[mode])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", FAMILIES["tet"][2])
def test_quad_search_is_the_single_lane_search(mode):
    """`tet_fast_exit_quad` (four lanes per history, data-parallel quad permutes): the drain kernel's boundary search.

    * the four lanes of a quad hold bit-identical results (one instruction stream on the same values; only the
      exchanged exits differ by lane);
    * wherever the quad certifies, it is held to the oracle like the single-lane search, same share floors;
    * where both certify, they name the same face;
    * in the reproducible build, whose promise is a history bit-defined in every kernel (and the drain kernel uses the
      quad), certificate, face and t equal the single-lane search's bit for bit."""
    table = cases("tet", mode)
    quad = quad_rows(table)
    bits = quad.view(np.uint64)
    assert np.array_equal(bits, np.broadcast_to(bits[:, :1, :], bits.shape)), np.flatnonzero((bits != bits[:, :1, :]).any(axis=(1, 2)))[:5]
    lead = np.ascontiguousarray(quad[:, 0, :])
    d = compare("tet", table, lead)
    print(f"\n[physics-device] quad search mode {mode}: length/R {d['dev_over_R']:.3g}; certified {d['certified'] / N:.4f}")
    assert_search(d, mode, TET_LEAST[mode])
    single = device_search(mode)
    both = (lead[:, 0] != 0) & (single[:, 0] != 0)
    assert both.any() and np.array_equal(lead[both, 1], single[both, 1])
    quad_r = np.ascontiguousarray(quad_rows(table, repro=True)[:, 0, :3]).view(np.uint64)
    single_r = np.ascontiguousarray(device_search(mode, repro=True)[:, :3]).view(np.uint64)
    differ = np.flatnonzero((quad_r != single_r).any(axis=1))
    assert differ.size == 0, (mode, differ.size, differ[:5], quad_rows(table, repro=True)[differ[:2], 0, :3], device_search(mode, repro=True)[differ[:2], :3])


# ---- inverse-CDF draws through the search guide, on the device --------------------------------------------------
def _guided_tables():
    rng = np.random.default_rng(7)
    x = np.linspace(-1, 1, 50000)
    flat = rng.uniform(0.0, 1.0, 20000)
    flat[rng.integers(0, flat.size, 8000)] = 0.0
    flat[:50] = 0.0
    tables = [("smooth", rng.uniform(0.5, 1.5, 4096), 10), ("peaked", np.exp(-(x / 0.01) ** 2) + 1e-9, 12),
              ("brackets of 8 to 64", np.ones(1 << 15), 10), ("flat stretches", flat, 9), ("flat stretches, fine guide", flat, 13)]
    return tables + [(f"tiny {n}", rng.uniform(0.1, 1.0, n), 4) for n in (1, 2, 3, 9, 17)]


def _guided_cases():
    """Every table through a guide built on the host (the case keeps the table's name) and through one built on the device."""
    tables = _guided_tables()
    return [pytest.param(n, w, b, 0, id=n) for n, w, b in tables] + [pytest.param(n, w, b, 1, id=n + ", device-built guide") for n, w, b in tables]


@pytest.mark.gpu
@pytest.mark.parametrize("name,weights,bits,guide_on_device", _guided_cases())
def test_device_guided_draw_is_the_bisection(name, weights, bits, guide_on_device):
    """`sample_cdf_guided` in its device form (address-space-1 loads of the cells and of the table) returns the index the
    host bisection `sample_cdf` returns, for every draw: random ones, the ends, and every table entry's own quantile
    with its two neighbours in floating point -- through a guide made by `build_guide_cells` on the host, and through one
    made in HBM by the engine's `build_guide_on_device`, the builder of every guide a run reads."""
    rng = np.random.default_rng(8)
    cdf = np.cumsum(weights)
    on = cdf / cdf[-1]
    u = np.concatenate([rng.uniform(0.0, 1.0, 20000), [0.0, 1.0 - 2.0 ** -53], on, np.nextafter(on, 0.0), np.nextafter(on, 2.0)])
    u = np.ascontiguousarray(u[(u >= 0.0) & (u <= 1.0)])
    guided_host, plain, longest = E.sample_cdf_both_ways(cdf, u, bits)
    if name == "peaked":
        assert longest > 64          # pivots, eight at once and the bisection of what is left
    if name == "brackets of 8 to 64":
        assert 8 <= longest <= 64
    L = device_lib()
    got = np.zeros(u.size, dtype=np.uint64)
    rc = L.r3d_devtest_guided(0, _dp(cdf), cdf.size, bits, _dp(u), u.size, got.ctypes.data_as(C.POINTER(C.c_uint64)), guide_on_device)
    assert rc == 0, L.r3d_devtest_last_error().decode()
    assert np.array_equal(got, plain), (name, np.flatnonzero(got != plain)[:5], longest)


@pytest.mark.gpu
def test_device_entries_refuse_what_they_cannot_run():
    L = device_lib()
    table = np.ascontiguousarray(cases("rot", 0)[:64])
    out = np.zeros((64, E.cases_width("rot", True)))
    calls = [lambda: L.r3d_devtest_eval(0, 2, 0, None, _dp(out), 64), lambda: L.r3d_devtest_eval(0, 2, 0, _dp(table), None, 64),
             lambda: L.r3d_devtest_eval(0, 5, 0, _dp(table), _dp(out), 64), lambda: L.r3d_devtest_eval(0, -1, 0, _dp(table), _dp(out), 64),
             lambda: L.r3d_devtest_quad(0, None, _dp(out), 4), lambda: L.r3d_devtest_quad(0, _dp(table), None, 4),
             lambda: L.r3d_devtest_guided(0, None, 8, 4, _dp(table), 8, None, 0),
             lambda: L.r3d_devtest_guided(0, _dp(table), 8, 4, None, 8, out.ctypes.data_as(C.POINTER(C.c_uint64)), 1)]
    for call in calls:
        assert call() == 1 and L.r3d_devtest_last_error().decode().startswith("r3d_devtest_")
    assert not out.any()
