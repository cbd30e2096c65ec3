"""The receiver collection ON THE DEVICE against a brute-force reference, arrival by arrival.

Between "the phonon is here" and "this bin gets this energy" the traversal kernel runs wave-cooperative code: the cell
lookup, the (arrival, candidate) pairs numbered by a prefix sum on the data-parallel primitives (`wave_scan_add`), dealt 64
per pass with the owner of each pair found by one `ds_permute` and a running maximum (`wave_scan_max`), the pole vote of
`sph_basis` under `cnt && type != P`, the open-addressed accumulators in LDS with their fall-through to HBM atomics and
the flush at the end of the block.  Whole runs (tests/test_gpu_parity.py) see it at the receiver layouts of the benchmark
models only.  Here tests/emul/collect_device.hip (`make devtest`) runs exactly that code over the receiver sets and arrival
tables of tests/collect_cases.py -- laid out so that each condition of the dealing is the deciding one somewhere -- in
every variant (TRACE x items from LDS / from HBM x 0, 32 or 256 accumulators, and the per-lane `collect()` of r3d_step.h),
in both builds, against that module's long-double reference without a grid and against the host build.

CAVEAT.  libr3d_collect_device.so is a sibling compilation of the engine's text under the engine's flags, and restates
three inline pieces of pool_body (the lookup, the LDS copy of the items, the flush; collect_device.hip names the lines):
an error of the source or of the compiler's handling of it shows here, one that only the traversal kernels' own register
allocation provokes does not.

Each test prints the largest energy deviation per variant on the scale of the bin's energy by type (LOG.md records them).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import collect_cases as K
import native_build
from test_rt_solve import TOL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD, GUARD_BYTE = 8, 0xA5
TRACE, LDS_ITEMS, PER_LANE, ACC_SHIFT = 1, 2, 4, 8
BUILDS = {"main": False, "repro": True}


def variants(lds_fits):
    """{label: variant word}: TRACE x {items in LDS, in HBM} x acc_bits {0, 5, 8}, and the per-lane form."""
    out = {}
    for trace in (0, TRACE):
        for lds in ((LDS_ITEMS, 0) if lds_fits else (0,)):
            for acc in (0, 5, 8):
                label = f"{'trace' if trace else 'plain'}-{'lds' if lds else 'hbm'}-acc{acc}"
                out[label] = trace | lds | (acc << ACC_SHIFT)
    out["per-lane"] = PER_LANE
    return out


def case_id(name):
    return name if K.CASES[name][3] else name + "(items-too-many-for-lds:hbm-only)"


CASE_PARAMS = [pytest.param(name, id=case_id(name)) for name in K.CASES]


@functools.lru_cache(maxsize=None)
def device_lib(repro=False):
    so = os.path.join(HERE, "emul", "libr3d_collect_device_repro.so" if repro else "libr3d_collect_device.so")
    lib = C.CDLL(native_build.make("devtest", missing=so))
    lib.r3d_devtest_last_error.restype = C.c_char_p
    lib.r3d_devtest_wave.restype = C.c_int
    lib.r3d_devtest_wave.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_uint64]
    lib.r3d_devtest_collect.restype = C.c_int
    lib.r3d_devtest_collect.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_double, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32] + [C.c_void_p] * 6
    return lib


def _guarded(n, dtype):
    return np.zeros(n + GUARD, dtype=dtype)


def raw_collect(repro, seis, time_per_bin, n_bins, arrivals, variant):
    """(return code, error text, the arrays WITH their guard words) of r3d_devtest_collect."""
    lib = device_lib(repro)
    seis, arrivals = np.ascontiguousarray(seis, dtype=np.float64), np.ascontiguousarray(arrivals, dtype=np.float64)
    n_seis, n_arr = seis.shape[0], arrivals.shape[0]
    slots = n_seis * n_bins if n_seis * n_bins < 2 ** 31 else 0        # (a refused call writes nothing)
    out = {"energy": _guarded(slots * 5, np.float64), "counts": _guarded(slots * 2, np.uint64), "catches": _guarded(n_arr, np.uint32),
           "hits": _guarded((n_arr + 63) // 64, np.uint32), "candidates": _guarded(n_arr, np.uint32), "grid": np.zeros(5, dtype=np.int64)}
    rc = lib.r3d_devtest_collect(0, seis.ctypes.data, n_seis, time_per_bin, n_bins, arrivals.ctypes.data, n_arr, variant,
                                 *[out[k].ctypes.data for k in ("energy", "counts", "catches", "hits", "candidates", "grid")])
    return rc, lib.r3d_devtest_last_error().decode(), out


@functools.lru_cache(maxsize=None)
def device_collect(name, label, repro):
    """One variant of one case on the device: the arrays without their guards (which are checked here); made once."""
    c = K.case(name)
    rc, text, out = raw_collect(repro, c.seis, c.time_per_bin, c.n_bins, c.arrivals, variants(c.lds_fits)[label])
    assert rc == 0, text
    for key in ("energy", "counts", "catches", "hits", "candidates"):
        guard = out[key][-GUARD:].view(np.uint8)
        assert np.all(guard == GUARD_BYTE), f"{name} {label}: the words behind `{key}` were written"
        out[key] = out[key][:-GUARD]
        out[key].setflags(write=False)
    out["energy"] = out["energy"].reshape(c.seis.shape[0], c.n_bins, 5)
    out["counts"] = out["counts"].reshape(c.seis.shape[0], c.n_bins, 2)
    return out


@functools.lru_cache(maxsize=None)
def host_collect(name):
    c = K.case(name)
    return K.host_collect(c.seis, c.time_per_bin, c.n_bins, c.arrivals)


# ---- the wave helpers ------------------------------------------------------------------------------------------
def wave_inputs():
    rng = np.random.default_rng(20261021)
    waves = [np.zeros(64), np.ones(64), np.full(64, 0xFFFF)]
    for lane in range(64):                                        # a single non-zero in each lane in turn (odd and even)
        w = np.zeros(64)
        w[lane] = 3 + lane
        waves.append(w)
    for lanes in ((15, 31, 47, 63), (16, 32, 48)):                # the row boundaries the broadcasts cross
        for value in (1, 0xFFFF):
            w = np.zeros(64)
            w[list(lanes)] = value
            waves.append(w)
    waves += list(rng.integers(0, 2 ** 20, (16, 64)))
    waves += list(rng.integers(0, 2 ** 20, (8, 64)) * (rng.uniform(0, 1, (8, 64)) < 0.2))   # (sparse: the identity of max)
    return np.array(waves, dtype=np.uint32)


@pytest.mark.parametrize("build", BUILDS)
def test_wave_scans_and_rank(build):
    """wave_scan_add, wave_scan_max and rank_in per wave against numpy.cumsum, maximum.accumulate and a popcount: exact."""
    lib, v = device_lib(BUILDS[build]), wave_inputs()
    add, mx, rank = np.zeros_like(v), np.zeros_like(v), np.zeros_like(v)
    rc = lib.r3d_devtest_wave(0, v.ctypes.data, add.ctypes.data, mx.ctypes.data, rank.ctypes.data, v.size)
    assert rc == 0, lib.r3d_devtest_last_error().decode()
    assert np.array_equal(add, np.cumsum(v, axis=1, dtype=np.uint32))
    assert np.array_equal(mx, np.maximum.accumulate(v, axis=1))
    odd = (v & 1).astype(np.uint32)
    assert np.array_equal(rank, np.cumsum(odd, axis=1, dtype=np.uint32) - odd)


# ---- the collection --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", CASE_PARAMS)
def test_device_collection_equals_the_reference(name, build):
    c, host, repro = K.case(name), host_collect(name), BUILDS[build]
    n_arr = c.arrivals.shape[0]
    wave_catches = np.add.reduceat(c.ref.catches.astype(np.uint64), np.arange(0, n_arr, 64))
    empty = c.ref.counts.sum(-1) == 0
    assert np.array_equal(host["counts"], c.ref.counts) and np.array_equal(host["catches"], c.ref.catches)
    report = []
    for label, word in variants(c.lds_fits).items():
        d = device_collect(name, label, repro)
        per_lane, trace = bool(word & PER_LANE), bool(word & TRACE)
        ok, dev = K.energies_within(d["energy"], c.ref.energy, TOL)
        report.append(f"{label} {dev:.3g}")
        assert np.array_equal(d["counts"], c.ref.counts), label
        assert np.array_equal(d["catches"], c.ref.catches if (trace or per_lane) else 0 * c.ref.catches), label
        assert np.array_equal(d["candidates"], 0 * host["candidates"] if per_lane else host["candidates"]), label
        assert np.array_equal(d["hits"], 0 * wave_catches if per_lane else wave_catches), label
        assert ok, (label, dev)
        assert np.all(d["energy"][empty] == 0.0) and not np.any(np.signbit(d["energy"][empty])), label
        assert np.array_equal(d["grid"], host["grid"]), label
    _, host_dev = K.energies_within(host["energy"], c.ref.energy, TOL)
    print(f"\n[collect-device] {name} {build}: energy deviation host {host_dev:.3g}; device " + ", ".join(report))


@pytest.mark.parametrize("name", [p for p in CASE_PARAMS if p.values[0] != "one-hot"])
def test_reproducible_build_defines_a_single_catch_to_the_bit(name):
    """A bin that took exactly one catch holds the same bits in every variant of the reproducible build, whatever kernel
    computed the contribution and whichever way it reached HBM."""
    c = K.case(name)
    single = c.ref.counts.sum(-1) == 1
    assert single.sum() > 20
    runs = {label: device_collect(name, label, True) for label in variants(c.lds_fits)}
    first = next(iter(runs.values()))["energy"][single].view(np.uint64)
    assert np.any(first != 0)
    for label, d in runs.items():
        assert np.array_equal(d["energy"][single].view(np.uint64), first), label


def test_the_device_sees_the_patterns():
    """The lane patterns of tests/test_collect.py's table, from the candidates the device kernel returns."""
    c = K.case("crowd-patterns")
    seen = K.lane_patterns(c.seis, c.arrivals, device_collect("crowd-patterns", "trace-hbm-acc5", False)["candidates"])
    assert all(seen.values()), [k for k, v in seen.items() if not v]


@pytest.mark.parametrize("build", BUILDS)
def test_refusals(build):
    """Null tables, a lane count that is no multiple of 64, a bin index that would not fit, accumulators the kernel is not
    built for, an item list too long for LDS: 1 with a text, nothing launched, nothing written."""
    lib, repro = device_lib(BUILDS[build]), BUILDS[build]
    v = np.zeros(128, dtype=np.uint32)
    outs = [np.full(128, 7, dtype=np.uint32) for _ in range(3)]
    ptrs = [o.ctypes.data for o in outs]
    assert lib.r3d_devtest_wave(0, v.ctypes.data, *ptrs, 100) == 1 and b"multiple of 64" in lib.r3d_devtest_last_error()
    assert lib.r3d_devtest_wave(0, None, *ptrs, 128) == 1 and b"null" in lib.r3d_devtest_last_error()
    assert lib.r3d_devtest_wave(0, v.ctypes.data, ptrs[0], None, ptrs[2], 128) == 1 and b"null" in lib.r3d_devtest_last_error()
    assert all(np.all(o == 7) for o in outs)
    c = K.case("one-mixed")

    def refused(text, seis=c.seis, n_bins=c.n_bins, arrivals=c.arrivals, variant=TRACE | (8 << ACC_SHIFT)):
        rc, said, out = raw_collect(repro, seis, c.time_per_bin, n_bins, arrivals, variant)
        assert rc == 1 and text in said, (rc, said)
        assert all(not np.any(a) for a in out.values())
    refused("n_seis * n_bins", n_bins=2 ** 31)
    refused("n_seis * n_bins", seis=np.repeat(c.seis, 2, axis=0), n_bins=2 ** 30)
    for acc in (1, 4, 9, 32):
        refused("acc_bits", variant=TRACE | (acc << ACC_SHIFT))
    refused("unknown variant", variant=PER_LANE | TRACE)
    bad_type = c.arrivals.copy()
    bad_type[5, 8] = 2
    refused("type", arrivals=bad_type)
    crowd = K.case("crowd-patterns")
    refused("does not fit in LDS", seis=crowd.seis, arrivals=crowd.arrivals, variant=LDS_ITEMS | (8 << ACC_SHIFT))
    rc = lib.r3d_devtest_collect(0, c.seis.ctypes.data, 1, 0.5, 64, None, 64, 0, *[None] * 6)
    assert rc == 1 and b"null" in lib.r3d_devtest_last_error()
