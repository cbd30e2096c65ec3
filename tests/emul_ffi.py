"""ctypes access to the TEST-ONLY host build of the kernel's per-lane code
(tests/emul/libr3d_emul.so).  See tests/emul/emul.cpp."""
import ctypes as C
import os

import native_build
from radiative3d_amd import _ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        native_build.make("emul")      # (every time: make knows what the library is built from)
        L = C.CDLL(os.path.join(_HERE, "emul", "libr3d_emul.so"))
        L.r3d_emul_run.restype = C.c_int
        L.r3d_emul_run.argtypes = [C.POINTER(_ffi.ModelDesc), C.c_uint64, C.c_uint64, C.c_uint64,
                                   C.POINTER(_ffi.Result), C.POINTER(_ffi.Final)]
        L.r3d_emul_set_volume.argtypes = [C.POINTER(_ffi.VolumeDesc), C.POINTER(C.c_uint32)]
        L.r3d_emul_face_class.restype = C.c_uint32
        L.r3d_emul_face_class.argtypes = [C.POINTER(_ffi.ModelDesc), C.c_int, C.c_int]
        L.r3d_emul_class_from_corners.restype = C.c_uint32
        L.r3d_emul_class_from_corners.argtypes = [C.POINTER(C.c_double), C.c_int]
        L.r3d_emul_sample_cdf.restype = None
        L.r3d_emul_sample_cdf.argtypes = [C.POINTER(C.c_double), C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.c_uint64,
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.r3d_emul_slow_moves.restype = C.c_ulonglong
        L.r3d_emul_slow_moves.argtypes = [C.c_int]
        L.r3d_emul_math.restype = C.c_double
        L.r3d_emul_math.argtypes = [C.c_int, C.c_double, C.c_double]
        _lib = L
    return _lib


def run_with_volume(model, n, vdesc, first_id=0, seed=0x5EED):
    import numpy as np
    shape = (2, int(vdesc.n_frames), int(vdesc.dims[2]), int(vdesc.dims[1]), int(vdesc.dims[0]))
    vol = np.zeros(shape, dtype=np.uint32)
    lib().r3d_emul_set_volume(C.byref(vdesc), vol.ctypes.data_as(C.POINTER(C.c_uint32)))
    try:
        res = run(model, n, first_id, seed)
    finally:
        lib().r3d_emul_set_volume(None, None)
    return res, vol


def run(model, n, first_id=0, seed=0x5EED, result=None, trace=False):
    res = result if result is not None else model.new_result()
    c = res._as_c()
    finals = (_ffi.Final * n)() if trace else None
    if lib().r3d_emul_run(model.desc_p, n, first_id, seed, C.byref(c), finals):
        raise RuntimeError("emul run failed")
    res._from_c(c)
    return (res, finals) if trace else res


F_SMOOTH, F_STEP = 16, 32


def class_from_corners(steps):
    """Pack-time class of a face from the signed velocity steps [(P, S), ...] at its corners."""
    flat = [x for pair in steps for x in pair]
    return int(lib().r3d_emul_class_from_corners((C.c_double * len(flat))(*flat), len(steps)))


def face_class(model, cell, face):
    return int(lib().r3d_emul_face_class(model.desc_p, cell, face))


def math_fn(which, x, y=0.0):
    """One of the kernel's lean elementary functions (tests/emul/emul.cpp r3d_emul_math)."""
    return float(lib().r3d_emul_math(which, float(x), float(y)))


def sample_cdf_both_ways(cdf, u, bits=0):
    """Indices drawn from the cumulative table `cdf` for the uniforms `u`: through the search guide's
    cells and by bisecting the whole table; and the longest bracket of the guide."""
    import numpy as np
    cdf = np.ascontiguousarray(cdf, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    a = np.empty(u.size, dtype=np.uint64)
    b = np.empty(u.size, dtype=np.uint64)
    longest = C.c_uint64(0)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    lib().r3d_emul_sample_cdf(cdf.ctypes.data_as(dp), cdf.size, bits, u.ctypes.data_as(dp), u.size,
                              a.ctypes.data_as(up), b.ctypes.data_as(up), C.byref(longest))
    return a, b, int(longest.value)


# ---- the case families of the per-lane physics, step by step (tests/emul/physics_cases.h) ----
# generate -> evaluate -> compare; the r3d_emul_* entries of the CPU tests run the three in one call on the host, a
# caller that evaluates a table elsewhere (tests/test_physics_device.py: on the device) takes the steps one by one.
CASE_FAMILIES = ("rt", "bend", "rot", "tet", "shell")       # the family numbers of physics_cases.h, in order


def cases_width(family, output=False):
    lib().r3d_cases_width.restype = C.c_int
    return int(lib().r3d_cases_width(CASE_FAMILIES.index(family), 1 if output else 0))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def cases_generate(family, mode, n, seed):
    """The n input rows that the family's r3d_emul_* entry runs for (mode, n, seed)."""
    import numpy as np
    table = np.zeros((n, cases_width(family)), dtype=np.float64)
    fn = getattr(lib(), f"r3d_cases_{family}_generate")
    fn.restype = None
    fn.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_double)]
    fn(mode, n, seed, _dp(table))
    return table


def cases_evaluate(family, table, flat_form=False):
    """The host build's output rows for the input rows `table`."""
    import numpy as np
    table = np.ascontiguousarray(table, dtype=np.float64)
    out = np.zeros((table.shape[0], cases_width(family, True)), dtype=np.float64)
    fn = getattr(lib(), f"r3d_cases_{family}_evaluate")
    fn.restype = None
    fn.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint64]
    fn(1 if flat_form else 0, _dp(table), _dp(out), table.shape[0])
    return out


def cases_compare(family, table, out, tol, margin, oracle):
    """An output table against the oracle's callback `oracle` (a ctypes function, or None where the family allows):
    (counters[8], dev[2], first_bad[16]) as the family's r3d_emul_* entry fills them."""
    import numpy as np
    table = np.ascontiguousarray(table, dtype=np.float64)
    out = np.ascontiguousarray(out, dtype=np.float64)
    assert table.shape == (out.shape[0], cases_width(family)) and out.shape[1] == cases_width(family, True)
    counters, dev, first = (C.c_uint64 * 8)(), (C.c_double * 2)(), (C.c_double * 16)()
    fn = getattr(lib(), f"r3d_cases_{family}_compare")
    fn.restype = None
    fn.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint64, C.c_double, C.c_double, C.POINTER(C.c_uint64),
                   C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]
    fn(_dp(table), _dp(out), table.shape[0], tol, margin, counters, dev, first, C.cast(oracle, C.c_void_p) if oracle else None)
    return list(counters), list(dev), list(first)
