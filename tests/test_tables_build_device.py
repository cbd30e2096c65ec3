"""The table-build kernels (radiative3d_amd/csrc/r3d_tables_build.hip) against a long-double reference, entry by entry.

tests/test_device_tables.py sees these kernels through a whole engine only: table lengths 20 * 4^degree (multiples of 16,
never shorter than a scan block), the icosahedron's directions (no pole, no psi = 0, no zeta = +-pi), the shipped
configurations' heterogeneity parameters, fp64 against the fp64 oracle at 1e-12 of the total, and guide_kernel,
toa_xyz_kernel and spol_cs_kernel not at all.  Here the builders themselves (r3d_tables_build.h) are driven through the
thin test-only entries of tests/emul/tables_device.hip, which is linked with the table OBJECT of each engine build
(`make devtest`: libr3d_tables_device.so has build/obj/main_tables.o, ..._repro.so has build/obj/repro_tables.o):

* lengths 1 .. 17 * 4096 + 1 around every edge of the scan (16 entries per work-item, 4096 per block, 256 per gsato block);
* directions that are no tessellation, theta = arccos of uniforms, phi uniform in (-pi, pi], the first 24 entries the
  products of psi in {0, pi, 1e-9, pi - 1e-9, pi/2, 1e-300} and zeta in {0, pi, -pi, pi/2};
* heterogeneity families from the shipped ones to forward-peaked ones, nu = 0, and one whose weights all fall under the
  1e-30 clamp; five moment tensors;
* the reference in numpy.longdouble (64-bit mantissa): the formulas of scatparams.cpp:75-194 and events.cpp:66-105 as
  oracle/r3d_tables_oracle.cpp restates them, prefix sums in long double by blocks (a chain of at most 2 * 256 additions
  of 2^-64: 3e-17, a thousandth of the bound below).  test_long_double_reference_is_the_oracles_formula holds it against
  the oracle where there is no GPU.

THE BOUND of a cumulative entry, P_k the exact prefix of the long-double weights:
    |cdf[k] - P_k| <= 1.01 * D * 2^-53 * P_k + (k + 1) * 4 * delta_w * w_max
D = 16 + 256 + ceil(n / 4096) is the longest chain of additions on the way to any entry (15 inside a work-item, 255 over
the work-items' totals, one to join them, ceil(n / 4096) - 1 over the block totals, one to add the block's offset): the
standard bound for sums of non-negative terms.  delta_w is the fp64 ORACLE's own largest deviation from the long-double
weights of that array on the same inputs, relative to the array's largest weight w_max; the device gets four times that
(its pow, sin and cos are other implementations with errors of the same few-ulp kind; the cancellation in the g_PS and
g_SP brackets is the formula's own).  cos_sums: the same two terms with D = 6 + 4 + ceil(n / 256) (six shuffles, four
waves, the blocks on the host; the first addition of each of the last two chains adds to zero and is exact, which pays
for the rounding of cos psi and of its product with the weight) and, the terms being signed, P = sum |cos psi| w.
Every test prints what it measured before it asserts (LOG.md records the figures).
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import native_build
from oracle import tables_ffi as T

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
U = 2.0 ** -53

LENGTHS = (1, 15, 16, 17, 255, 4095, 4096, 4097, 3 * 4096 + 17, 17 * 4096 + 1)
N_MAX = max(LENGTHS)
PSI_EDGES = (0.0, math.pi, 1e-9, math.pi - 1e-9, math.pi / 2, 1e-300)
ZETA_EDGES = (0.0, math.pi, -math.pi, math.pi / 2)
HET = {"shipped, a 0.2": [0.8, 0.01, 0.2, 0.2, 4.83, 1.73],
       "shipped, a 1": [0.8, 0.01, 1.0, 0.5, 3.46, 1.763],
       "forward-peaked": [0.8, 0.05, 10, 0.8, 200, 1.73],
       "very forward-peaked": [0.8, 0.05, 50, 2.0, 2000, 1.73],     # (the total of one table ~5e-15 of another's)
       "nu = 0": [0.0, 0.01, 0.5, 0.3, 5, 1.8],
       "all under the clamp": [0.8, 1e-9, 1e-3, 0.1, 1e-3, 1.73]}
MIN_THETA, MAX_THETA = 0.0000001, math.pi - 0.0000001                   # host/model.cpp (phonons.cpp:34-35)
BUILDS = [pytest.param(False, id="engine"), pytest.param(True, id="repro")]


@functools.lru_cache(maxsize=None)
def moments():
    couple, _ = T.moment_tensor("SDR", (125, 40, 90, 0.0, 1.0), 0, 6371.0, (0.0, 0.0, 0.0))   # (the configurations' "eq")
    return {"double couple": tuple(couple), "explosion": (1., 1., 1., 0., 0., 0.), "vertical dipole": (0., 0., 1., 0., 0., 0.),
            "xy only": (0., 0., 0., 1., 0., 0.), "zero": (0.,) * 6}


MOMENT_NAMES = ("double couple", "explosion", "vertical dipole", "xy only", "zero")


# ---- inputs ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def directions():
    """The N_MAX (theta, phi) pairs; a table of n entries takes the first n.  Made once, never written to."""
    rng = np.random.default_rng(1)
    toa = np.empty((N_MAX, 2))
    toa[:, 0] = np.arccos(rng.uniform(-1.0, 1.0, N_MAX))
    toa[:, 1] = math.pi - 2.0 * math.pi * rng.uniform(0.0, 1.0, N_MAX)          # (-pi, pi]
    edges = [(p, z) for z in ZETA_EDGES for p in PSI_EDGES]                     # (n = 15 .. 17 hold three zetas)
    toa[:len(edges)] = edges
    assert np.all((toa[:, 0] >= 0) & (toa[:, 0] <= math.pi) & (toa[:, 1] >= -math.pi) & (toa[:, 1] <= math.pi))
    toa.setflags(write=False)
    return toa


def psdf_numer(het):
    """include/r3d.h: 8 pi^1.5 eps^2 a^3 Gamma(kappa + 1.5) / Gamma(kappa) (in the host's order, scatparams.hpp)."""
    _, eps, a, kappa, _, _ = het
    return (8. * math.pow(math.pi, 1.5) * eps * eps * a * a * a) * math.gamma(kappa + 1.5) / math.gamma(kappa)


# ---- the long-double reference -----------------------------------------------------------------------------------
def ld_gsato(het, numer, toa):
    """ScatterParams::GSATO / XSATO / PSATO (scatparams.cpp:75-194) in long double: (weights[4, n] BEFORE the clamp,
    xss_zeta, xss_psi).  Every constant is the programs' own double, taken exactly."""
    nu, _, a, kappa, el, gam0 = (LD(x) for x in het)
    numer, pi = LD(numer), LD(math.pi)
    psi, zeta = toa[:, 0].astype(LD), toa[:, 1].astype(LD)
    g2 = gam0 * gam0
    cpsi, c2psi, spsi, czeta, szeta = np.cos(psi), np.cos(2 * psi), np.sin(psi), np.cos(zeta), np.sin(zeta)
    spsi2 = spsi * spsi
    xpp = (1 / g2) * (nu * (-1 + cpsi + (2 / g2) * spsi2) - 2 + (4 / g2) * spsi2)
    xps = -spsi * (nu * (1 - (2 / gam0) * cpsi) - (4 / gam0) * cpsi)
    xsp = (1 / g2) * spsi * czeta * (nu * (1 - (2 / gam0) * cpsi) - (4 / gam0) * cpsi)
    xss_psi = czeta * (nu * (cpsi - c2psi) - 2 * c2psi)
    xss_zeta = szeta * (nu * (cpsi - 1) + 2 * cpsi)

    def psato(m):
        return numer / np.power(1 + a * a * m * m, kappa + LD(1.5))

    scale = (el * el) * (el * el) / (4 * pi)
    pm = psato((el / gam0) * np.sqrt(1 + g2 - 2 * gam0 * cpsi))
    w = np.stack([scale * (xpp * xpp) * psato((2 * el / gam0) * np.sin(psi / 2)),
                  (1 / gam0) * scale * (xps * xps) * pm,
                  gam0 * scale * (xsp * xsp) * pm,
                  scale * (xss_psi * xss_psi + xss_zeta * xss_zeta) * psato(2 * el * np.sin(psi / 2))])
    return w, xss_zeta, xss_psi


def ld_source(mt, toa):
    """ShearDislocation's P, SH, SV patterns (events.cpp:66-105) in long double: weights[3, n]."""
    mxx, myy, mzz, mxy, mxz, myz = (LD(x) for x in mt)
    th, az = toa[:, 0].astype(LD), toa[:, 1].astype(LD)
    st, ct, sa, ca, s2a, c2a = np.sin(th), np.cos(th), np.sin(az), np.cos(az), np.sin(2 * az), np.cos(2 * az)
    horiz = mxx * ca * ca + mxy * s2a + myy * sa * sa - mzz
    vert = mxz * ca + myz * sa
    pp = st * st * horiz + 2 * st * ct * vert + mzz
    sh = st * (LD(0.5) * s2a * (myy - mxx) + c2a * mxy) + ct * (ca * myz - sa * mxz)
    sv = st * ct * horiz + (1 - 2 * st * st) * vert
    return np.stack([pp * pp, sh * sh, sv * sv])


def ld_prefix(w):
    """Inclusive prefix sums along the last axis in long double, by blocks of 256: no entry is further than 2 * 256
    additions of 2^-64 from its terms."""
    w = np.atleast_2d(w)
    rows, n = w.shape
    blocks = -(-n // 256)
    padded = np.zeros((rows, blocks * 256), dtype=LD)
    padded[:, :n] = w
    inner = np.cumsum(padded.reshape(rows, blocks, 256), axis=2)
    before = np.cumsum(inner[:, :, -1], axis=1) - inner[:, :, -1]
    return (inner + before[:, :, None]).reshape(rows, -1)[:, :n]


def ld_sum(x):
    return ld_prefix(x)[0, -1]


def clamped(w_raw):
    """The reference's "< 1e-30 -> 0"; the clamp may not decide a comparison: no weight within 1 +- 1e-9 of it."""
    edge = LD(1e-30)
    assert not np.any(np.abs(w_raw / edge - 1) <= LD(1e-9)), "a reference weight sits on the 1e-30 clamp"
    return np.where(w_raw < edge, LD(0), w_raw)


def oracle_gsato_rows(het, toa):
    """The fp64 oracle's GSATO per direction: rows of gpp, gps, gsp, gss, spol."""
    L, dp = T.lib(), C.POINTER(C.c_double)
    out = np.zeros((len(toa), 5))
    h = (C.c_double * 6)(*het)
    base, fn = out.ctypes.data, L.r3d_oracle_gsato
    for k, (theta, phi) in enumerate(toa.tolist()):
        fn(h, theta, phi, C.cast(base + 40 * k, dp))
    return out


def oracle_source_rows(mt, toa):
    """The fp64 oracle's source weights per direction (r3d_oracle_source on tables of one entry): rows of P, SH, SV."""
    L, dp = T.lib(), C.POINTER(C.c_double)
    toa = np.ascontiguousarray(toa)
    out = np.zeros((len(toa), 3))
    m, whole = (C.c_double * 6)(*mt), (C.c_double * 3)()
    ptrs = (dp * 3)()
    tbase, obase, fn = toa.ctypes.data, out.ctypes.data, L.r3d_oracle_source
    for k in range(len(toa)):
        for c in range(3):
            ptrs[c] = C.cast(obase + 24 * k + 8 * c, dp)
        fn(m, C.cast(tbase + 16 * k, dp), 1, ptrs, whole)
    return out


@functools.lru_cache(maxsize=None)
def scatterer_reference(family):
    """(long-double weights[4, N_MAX] after the clamp, (xss_zeta, xss_psi), |oracle - reference|[4, N_MAX], the oracle's spol)."""
    het, toa = HET[family], directions()
    w_raw, xz, xp = ld_gsato(het, psdf_numer(het), toa)
    w = clamped(w_raw)
    rows = oracle_gsato_rows(het, toa)
    return w, (xz, xp), np.abs(rows[:, :4].T.astype(LD) - w), rows[:, 4]


@functools.lru_cache(maxsize=None)
def source_reference(name):
    mt, toa = moments()[name], directions()
    w = ld_source(mt, toa)
    return w, np.abs(oracle_source_rows(mt, toa).T.astype(LD) - w)


def delta_w(w, oracle_off, n):
    """Per array: (the oracle's largest deviation over the first n weights relative to their largest, that largest)."""
    w_max = np.max(w[:, :n], axis=1)
    off = np.max(oracle_off[:, :n], axis=1)
    return np.where(w_max > 0, off / np.where(w_max > 0, w_max, 1), LD(0)), w_max


def cdf_bounds(w, oracle_off, n, factor=4, chain=None):
    """(P[rows, n], the bound of every entry[rows, n], delta_w[rows]) for tables of the first n weights."""
    P = ld_prefix(w[:, :n])
    d, w_max = delta_w(w, oracle_off, n)
    D = chain if chain is not None else 16 + 256 + -(-n // 4096)
    k1 = np.arange(1, n + 1).astype(LD)
    return P, LD(1.01) * D * LD(U) * P + k1[None, :] * (factor * d * w_max)[:, None], d


def assert_cumulative(cdf, totals, w, oracle_off, n, what):
    """The assertions on a set of cumulative tables cdf[rows, n]; returns (delta_w, the largest share of the bound used)."""
    P, bound, d = cdf_bounds(w, oracle_off, n)
    off = np.abs(cdf.astype(LD) - P)
    share = np.max(np.where(bound > 0, off / np.where(bound > 0, bound, 1), np.where(off > 0, np.inf, 0)), axis=1)
    rel = np.max(np.where(P > 0, off / np.where(P > 0, P, 1), 0), axis=1)
    print(f"\n[tables-device] {what}, n {n}: oracle delta_w {np.array2string(d.astype(float), precision=3)}; "
          f"device |cdf - P| / P at most {np.array2string(rel.astype(float), precision=3)}, "
          f"share of the bound used {np.array2string(share.astype(float), precision=3)}")
    for c in range(cdf.shape[0]):
        assert np.all(np.diff(cdf[c]) >= 0), (what, c, "not non-decreasing")
        assert totals[c] == cdf[c, -1], (what, c)
        bad = np.flatnonzero(~(off[c] <= bound[c]))
        assert bad.size == 0, (what, c, bad[:5], cdf[c, bad[:5]], P[c, bad[:5]], bound[c, bad[:5]])
    return d, share


# ---- the device entries ------------------------------------------------------------------------------------------
_dp = C.POINTER(C.c_double)


def p(a):
    return a.ctypes.data_as(_dp)


@functools.lru_cache(maxsize=None)
def device_lib(repro=False):
    so = os.path.join(HERE, "emul", "libr3d_tables_device_repro.so" if repro else "libr3d_tables_device.so")
    L = C.CDLL(native_build.make("devtest", missing=so))
    L.r3d_devtest_last_error.restype = C.c_char_p
    for name, args in [("toa", [C.c_int, C.c_int, C.c_uint64, _dp]),
                       ("toa_xyz", [C.c_int, _dp, C.c_uint64, C.c_double, C.c_double, _dp]),
                       ("scatterer", [C.c_int, _dp, C.c_double, _dp, C.c_uint64, _dp, _dp, _dp, _dp]),
                       ("source", [C.c_int, _dp, _dp, C.c_uint64, _dp, _dp]),
                       ("spol_cs", [C.c_int, _dp, C.c_uint64, _dp]),
                       ("guide", [C.c_int, _dp, C.c_uint64, C.c_uint32, C.c_void_p]),
                       ("host_guide", [_dp, C.c_uint64, C.c_uint32, C.c_void_p])]:
        fn = getattr(L, "r3d_devtest_" + name)
        fn.restype, fn.argtypes = C.c_int, args
    L.r3d_devtest_guide_bits_for.restype, L.r3d_devtest_guide_bits_for.argtypes = C.c_uint32, [C.c_uint64]
    return L


def ok(L, rc):
    assert rc == 0, L.r3d_devtest_last_error().decode()


@functools.lru_cache(maxsize=None)
def device_scatterer(repro, family, n):
    """(cdf[4, n], spol[n], totals[4], cos_sums[4]) of build_scatterer_tables; made once per case, never written to."""
    L, het = device_lib(repro), np.array(HET[family], dtype=np.float64)
    toa = np.ascontiguousarray(directions()[:n])
    cdf, spol, totals, cos_sums = np.full((4, n), np.nan), np.full(n, np.nan), np.full(4, np.nan), np.full(4, np.nan)
    ok(L, L.r3d_devtest_scatterer(0, p(het), psdf_numer(HET[family]), p(toa), n, p(cdf), p(spol), p(totals), p(cos_sums)))
    for a in (cdf, spol, totals, cos_sums):
        a.setflags(write=False)
    return cdf, spol, totals, cos_sums


@functools.lru_cache(maxsize=None)
def device_source(repro, name, n):
    L, mt = device_lib(repro), np.array(moments()[name], dtype=np.float64)
    toa = np.ascontiguousarray(directions()[:n])
    cdf, totals = np.full((3, n), np.nan), np.full(3, np.nan)
    ok(L, L.r3d_devtest_source(0, p(mt), p(toa), n, p(cdf), p(totals)))
    cdf.setflags(write=False), totals.setflags(write=False)
    return cdf, totals


def guides(L, cdf, bits, device=True):
    """The 2^bits cells as bytes[2^bits, 64]."""
    cdf = np.ascontiguousarray(cdf, dtype=np.float64)
    cells = np.full((1 << bits, 64), 0xA5, dtype=np.uint8)
    if device:
        ok(L, L.r3d_devtest_guide(0, p(cdf), cdf.size, bits, cells.ctypes.data))
    else:
        ok(L, L.r3d_devtest_host_guide(p(cdf), cdf.size, bits, cells.ctypes.data))
    return cells


def angle_off(a, b):
    """|a - b| as angles modulo 2 pi (in long double: the difference is taken before it is folded)."""
    d = np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD))
    two_pi = 2 * LD("3.14159265358979323846264338327950288")
    d = np.where(d > two_pi / 2, np.abs(d - two_pi), d)
    return d


# ---- CPU: the reference itself ------------------------------------------------------------------------------------
#: the oracle evaluates in fp64 what the reference evaluates in long double: some twenty roundings on the way to a
#: weight, the eight of the power's base amplified by its exponent kappa + 1.5 <= 3.5, and Gamma() from another
#: library: under 64 units in the last place of the array's largest weight (what was seen: 4e-15 at the most)
ORACLE_ULPS = 64


@pytest.mark.parametrize("family", list(HET))
def test_long_double_reference_is_the_oracles_formula(family):
    """The long-double GSATO against the fp64 oracle on the test's own directions: weights to ORACLE_ULPS of the array's
    largest, the clamp at the same entries, spol to the project's 1e-9 wherever the S -> S pattern is not zero, and the
    oracle's own cumulative tables (summed in index order: a chain of n) within the bound with ITS delta_w, not four times."""
    w, (xz, xp), off, spol_o = scatterer_reference(family)
    d, w_max = delta_w(w, off, N_MAX)
    print(f"\n[tables-device] {family}: oracle delta_w {np.array2string(d.astype(float), precision=3)} "
          f"w_max {np.array2string(w_max.astype(float), precision=3)}")
    assert np.all(d <= ORACLE_ULPS * U), d
    rows = oracle_gsato_rows(HET[family], directions()[:4096])
    assert np.array_equal(rows[:, :4].T == 0, w[:, :4096] == 0)
    if family == "all under the clamp":
        assert not w.any()
    else:
        assert np.all(w_max > 0)
    known = (xz * xz + xp * xp) != 0
    assert known.sum() > 0.99 * N_MAX
    assert np.max(angle_off(spol_o, np.arctan2(xz, xp))[known]) < 1e-9
    for n in (17, 4097):
        toa = directions()[:n]
        o = T.scatterer(HET[family], toa)
        P, bound, _ = cdf_bounds(w, off, n, factor=1, chain=n)
        assert np.all(np.abs(o["cdf"].astype(LD) - P) <= bound)


@pytest.mark.parametrize("name", MOMENT_NAMES)
def test_long_double_source_reference_is_the_oracles_formula(name):
    """The long-double radiation patterns against the fp64 oracle: each weight is the square of a sum of at most six terms
    no larger than 2 sum |M_ij|, every term a few roundings from exact: ORACLE_ULPS of (2 sum |M_ij|)^2 (an explosion's
    SH and SV patterns are nothing BUT rounding, so the array's own largest weight is no scale here)."""
    w, off = source_reference(name)
    scale = (2 * sum(abs(x) for x in moments()[name])) ** 2
    print(f"\n[tables-device] source {name}: oracle off by at most {np.array2string(np.max(off, axis=1).astype(float), precision=3)}, "
          f"largest weights {np.array2string(np.max(w, axis=1).astype(float), precision=3)}")
    assert np.all(off <= ORACLE_ULPS * U * scale)
    for n in (17, 4097):
        cdf, _ = T.source(moments()[name], directions()[:n])
        P, bound, _ = cdf_bounds(w, off, n, factor=1, chain=n)
        assert np.all(np.abs(cdf.astype(LD) - P) <= bound)
    if name == "double couple":          # (the closed form tests/test_tables_oracle.py holds the oracle to: P : S = 2 : 3)
        total = ld_prefix(w)[:, -1]
        assert float(total[0] / (total[1] + total[2])) == pytest.approx(2 / 3, rel=0.02)


def test_prefix_sums_by_blocks_are_the_exact_sums():
    rng = np.random.default_rng(3)
    x = rng.uniform(0.0, 1.0, (2, 70001)) * 10.0 ** rng.integers(-20, 5, (2, 70001))
    got = ld_prefix(x.astype(LD))
    for k in (0, 255, 256, 257, 4096, 70000):
        for r in range(2):
            # (math.fsum is the exact sum ROUNDED to double)
            assert abs(got[r, k] - LD(math.fsum(x[r, :k + 1]))) <= (LD(U) + 600 * LD(2.0) ** -64) * got[r, k]


# ---- GPU: cumulative tables ----------------------------------------------------------------------------------------
def sampled_weight_deviation(repro, family):
    """The device's own delta_w where it can be read exactly: a table of ONE entry is its weight (0 + w), so 256 tables of one
    entry (the 24 edge directions and 232 others) give 256 device weights; beside the oracle's deviation on the same 256."""
    L, het = device_lib(repro), np.array(HET[family], dtype=np.float64)
    w, _, off, _ = scatterer_reference(family)
    idx = np.concatenate([np.arange(24), np.arange(24, N_MAX, (N_MAX - 24) // 232)[:232]])
    got = np.zeros((4, idx.size))
    cdf, spol, totals, cos_sums = np.zeros(4), np.zeros(1), np.zeros(4), np.zeros(4)
    for j, k in enumerate(idx):
        toa = np.ascontiguousarray(directions()[k:k + 1])
        ok(L, L.r3d_devtest_scatterer(0, p(het), psdf_numer(HET[family]), p(toa), 1, p(cdf), p(spol), p(totals), p(cos_sums)))
        got[:, j] = cdf
    w_max = np.max(w[:, idx], axis=1)
    scale = np.where(w_max > 0, w_max, 1)
    return np.max(np.abs(got.astype(LD) - w[:, idx]), axis=1) / scale, np.max(off[:, idx], axis=1) / scale


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("family", list(HET))
@pytest.mark.parametrize("repro", BUILDS)
def test_scatterer_tables_are_the_long_double_prefix_sums(repro, family, n):
    w, (xz, xp), off, _ = scatterer_reference(family)
    cdf, spol, totals, cos_sums = device_scatterer(repro, family, n)
    assert_cumulative(cdf, totals, w, off, n, f"{family} ({'repro' if repro else 'engine'})")
    if family == "all under the clamp":
        assert not cdf.any() and not totals.any() and not cos_sums.any()
    # the dipole sums
    cpsi = np.cos(directions()[:n, 0].astype(LD))
    d, w_max = delta_w(w, off, n)
    D = 6 + 4 + -(-n // 256)
    for c in range(4):
        want, absolute = ld_sum(cpsi * w[c, :n]), ld_sum(np.abs(cpsi) * w[c, :n])
        bound = LD(1.01) * D * LD(U) * absolute + n * 4 * d[c] * w_max[c]
        print(f"[tables-device] cos_sums[{c}] off by {float(abs(cos_sums[c] - want)):.3g}, bound {float(bound):.3g}")
        assert abs(cos_sums[c] - want) <= bound, (family, n, c, cos_sums[c], want, bound)
    # the S -> S polarisation angle, wherever the pattern it is the direction of is not zero
    known = (xz[:n] * xz[:n] + xp[:n] * xp[:n]) != 0
    worst = np.max(angle_off(spol, np.arctan2(xz[:n], xp[:n]))[known]) if known.any() else 0
    print(f"[tables-device] spol off by at most {float(worst):.3g} over {known.sum()} of {n}")
    assert np.all(np.isfinite(spol)) and np.all(np.abs(spol) <= math.pi) and worst < 1e-9
    if n == N_MAX:
        dev, orc = sampled_weight_deviation(repro, family)
        print(f"[tables-device] {family} ({'repro' if repro else 'engine'}), 256 single weights: device delta_w "
              f"{np.array2string(dev.astype(float), precision=3)} oracle {np.array2string(orc.astype(float), precision=3)}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", MOMENT_NAMES)
@pytest.mark.parametrize("repro", BUILDS)
def test_source_tables_are_the_long_double_prefix_sums(repro, name, n):
    w, off = source_reference(name)
    cdf, totals = device_source(repro, name, n)
    assert_cumulative(cdf, totals, w, off, n, f"source {name} ({'repro' if repro else 'engine'})")
    if name == "zero":
        assert not cdf.any() and not totals.any()


# ---- GPU: take-off set, direction vectors, polarisation pairs ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("degree", range(4))
@pytest.mark.parametrize("repro", BUILDS)
def test_generated_take_off_set_is_the_oracles(repro, degree):
    L, n = device_lib(repro), 20 * 4 ** degree
    toa = np.full((n, 2), np.nan)
    ok(L, L.r3d_devtest_toa(0, degree, n, p(toa)))
    want = T.toa(degree)
    off_theta, off_phi = np.max(np.abs(toa[:, 0] - want[:, 0])), float(np.max(angle_off(toa[:, 1], want[:, 1])))
    print(f"\n[tables-device] take-off set of degree {degree}: theta off by {off_theta:.3g}, phi by {off_phi:.3g}")
    assert off_theta < 1e-14 and off_phi < 1e-14


def xyz_input(min_theta, max_theta):
    """The first 4113 directions, then a twin of every direction outside [min_theta, max_theta] with theta ON the clamp
    value and the same phi, then the two clamp values themselves at phi = 0."""
    toa = directions()[:4113]
    low, high = toa[toa[:, 0] < min_theta], toa[toa[:, 0] > max_theta]
    twins = np.concatenate([np.column_stack([np.full(len(low), min_theta), low[:, 1]]),
                            np.column_stack([np.full(len(high), max_theta), high[:, 1]])])
    return np.ascontiguousarray(np.concatenate([toa, twins, [[min_theta, 0.0], [max_theta, 0.0]]])), len(low), len(high)


@pytest.mark.gpu
@pytest.mark.parametrize("min_theta,max_theta", [(MIN_THETA, MAX_THETA), (0.3, 2.5), (0.0, math.pi)])
@pytest.mark.parametrize("repro", BUILDS)
def test_direction_vectors_are_cos_and_sin_of_the_clamped_angles(repro, min_theta, max_theta):
    L = device_lib(repro)
    toa, n_low, n_high = xyz_input(min_theta, max_theta)
    n, m = len(toa), 4113
    xyz = np.full((n, 4), np.nan)
    ok(L, L.r3d_devtest_toa_xyz(0, p(toa), n, min_theta, max_theta, p(xyz)))
    th, ph = np.clip(toa[:, 0], min_theta, max_theta).astype(LD), toa[:, 1].astype(LD)
    want = np.column_stack([np.cos(th), np.cos(ph), np.sin(ph), np.sin(th)])
    worst = float(np.max(np.abs(xyz.astype(LD) - want)))
    print(f"\n[tables-device] direction vectors, theta in [{min_theta}, {max_theta}]: off by at most {worst:.3g}; "
          f"{n_low} rows below, {n_high} above")
    assert worst <= 1e-14
    if min_theta > 0:      # theta = 0, 1e-300, 1e-9 and pi, pi - 1e-9 of the edge directions (four zetas each), at the least
        assert n_low >= 4 and n_high >= 4
    below, above = np.flatnonzero(toa[:m, 0] < min_theta), np.flatnonzero(toa[:m, 0] > max_theta)
    clamped_rows = xyz[np.concatenate([below, above])].view(np.uint64)
    assert np.array_equal(clamped_rows, xyz[m:m + n_low + n_high].view(np.uint64))
    for rows, edge in ((below, n - 2), (above, n - 1)):
        assert np.array_equal(xyz[rows][:, [0, 3]].view(np.uint64), np.tile(xyz[edge, [0, 3]], (len(rows), 1)).view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("repro", BUILDS)
def test_polarisation_pairs_are_cos_and_sin_of_the_angles(repro):
    L = device_lib(repro)
    _, (xz, xp), _, _ = scatterer_reference("shipped, a 1")
    spol = np.concatenate([np.arctan2(xz, xp).astype(np.float64)[:3 * 4096 + 17],
                           [0.0, -0.0, math.pi, -math.pi, math.pi / 2, -math.pi / 2, 1e-300, -1e-300, 1e-9]])
    spol = np.ascontiguousarray(spol)
    for n in (1, 255, 256, 257, spol.size):
        cs = np.full((n, 2), np.nan)
        ok(L, L.r3d_devtest_spol_cs(0, p(spol[spol.size - n:]), n, p(cs)))
        a = spol[spol.size - n:].astype(LD)
        worst = float(np.max(np.abs(cs.astype(LD) - np.column_stack([np.cos(a), np.sin(a)]))))
        print(f"\n[tables-device] polarisation pairs, n {n}: off by at most {worst:.3g}")
        assert worst <= 1e-14


# ---- GPU: the search guides -------------------------------------------------------------------------------------------
def assert_same_guide(L, cdf, bits, what):
    dev, host = guides(L, cdf, bits), guides(L, cdf, bits, device=False)
    differ = np.flatnonzero((dev != host).any(axis=1))
    assert differ.size == 0, (what, bits, differ.size, differ[:5], dev[differ[:2]].view(np.uint32)[:, :2], host[differ[:2]].view(np.uint32)[:, :2])


def guide_families():
    from test_physics_device import _guided_tables
    return [(name, np.cumsum(weights), bits) for name, weights, bits in _guided_tables()] + \
           [("all zero", np.zeros(100), 4), ("all zero, fine guide", np.zeros(100), 9), ("one zero", np.zeros(1), 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("repro", BUILDS)
def test_device_guide_is_the_host_guide_on_hard_tables(repro):
    """The table families of tests/test_guide_cells.py (smooth; peaked, brackets beyond 64 entries; brackets of 32; flat
    stretches with leading zeros, also with more cells than distinct values; n = 1, 2, 3, 9, 17) and all-zero tables."""
    L = device_lib(repro)
    for name, cdf, bits in guide_families():
        assert_same_guide(L, cdf, bits, name)
        cells = guides(L, cdf, bits)
        k = cells.view(np.uint32)[:, :2]
        assert k[0, 0] == 0 and np.all(k[:, 0] <= k[:, 1]) and np.all(k[1:, 0] == k[:-1, 1]) and k[-1, 1] <= cdf.size - 1, name


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("repro", BUILDS)
def test_device_guide_is_the_host_guide_on_the_built_tables(repro, n):
    """Every cumulative table built above (six scatterers of four, five sources of three), guides of 2^4 cells, of the
    engine's width for n entries and of 2^13."""
    L = device_lib(repro)
    widths = sorted({4, int(L.r3d_devtest_guide_bits_for(n)), 13})
    for bits in widths:
        for family in HET:
            for c, cdf in enumerate(device_scatterer(repro, family, n)[0]):
                assert_same_guide(L, cdf, bits, (family, c, n))
        for name in MOMENT_NAMES:
            for c, cdf in enumerate(device_source(repro, name, n)[0]):
                assert_same_guide(L, cdf, bits, (name, c, n))


# ---- GPU: refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("repro", BUILDS)
def test_table_entries_refuse_what_they_cannot_build(repro):
    """n = 0, a degree outside 0 .. 12, n != 20 * 4^degree, null and oversized tables: 1, an error text, nothing written."""
    L = device_lib(repro)
    toa = np.ascontiguousarray(directions()[:64])
    het, mt = np.array(HET["shipped, a 1"]), np.array(moments()["double couple"])
    out = np.zeros((4, 64 * 4))
    small = [np.zeros(4), np.zeros(4)]
    cells = np.zeros((16, 64), dtype=np.uint8)
    too_many = (1 << 24) + 1
    calls = [lambda: L.r3d_devtest_toa(0, -1, 20, p(out)), lambda: L.r3d_devtest_toa(0, 13, 20 * 4 ** 13, p(out)),
             lambda: L.r3d_devtest_toa(0, 1, 20, p(out)), lambda: L.r3d_devtest_toa(0, 1, 81, p(out)),
             lambda: L.r3d_devtest_toa(0, 0, 0, p(out)), lambda: L.r3d_devtest_toa(0, 1, 80, None),
             lambda: L.r3d_devtest_toa_xyz(0, p(toa), 0, MIN_THETA, MAX_THETA, p(out)),
             lambda: L.r3d_devtest_toa_xyz(0, None, 64, MIN_THETA, MAX_THETA, p(out)),
             lambda: L.r3d_devtest_toa_xyz(0, p(toa), too_many, MIN_THETA, MAX_THETA, p(out)),
             lambda: L.r3d_devtest_scatterer(0, p(het), 1.0, p(toa), 0, p(out), p(out[1]), p(small[0]), p(small[1])),
             lambda: L.r3d_devtest_scatterer(0, p(het), 1.0, None, 64, p(out), p(out[1]), p(small[0]), p(small[1])),
             lambda: L.r3d_devtest_scatterer(0, p(het), 1.0, p(toa), too_many, p(out), p(out[1]), p(small[0]), p(small[1])),
             lambda: L.r3d_devtest_source(0, p(mt), p(toa), 0, p(out), p(small[0])),
             lambda: L.r3d_devtest_source(0, p(mt), p(toa), 64, None, p(small[0])),
             lambda: L.r3d_devtest_spol_cs(0, p(toa), 0, p(out)), lambda: L.r3d_devtest_spol_cs(0, p(toa), 64, None),
             lambda: L.r3d_devtest_guide(0, p(toa), 0, 4, cells.ctypes.data), lambda: L.r3d_devtest_guide(0, p(toa), 64, 25, cells.ctypes.data),
             lambda: L.r3d_devtest_guide(0, None, 64, 4, cells.ctypes.data), lambda: L.r3d_devtest_guide(0, p(toa), 64, 4, None),
             lambda: L.r3d_devtest_host_guide(p(toa), 0, 4, cells.ctypes.data), lambda: L.r3d_devtest_host_guide(None, 64, 4, cells.ctypes.data)]
    for k, call in enumerate(calls):
        assert call() == 1 and L.r3d_devtest_last_error().decode().startswith(("r3d_devtest_", "build_")), k
    assert not out.any() and not small[0].any() and not small[1].any() and not cells.any()
