"""ctypes mirror of include/r3d.h and include/r3d_host.h.

Only plain C crosses the boundary; these Structure classes restate the POD
layouts field for field.  tests/test_abi.py checks sizes against the compiled
libraries.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.join(_HERE, "lib")
REPO = os.path.dirname(_HERE)

R3D_CELL_CYLINDER, R3D_CELL_TETRA, R3D_CELL_SPHERESHELL = 0, 1, 2
R3D_FACE_COLLECT, R3D_FACE_REFLECT, R3D_FACE_ADJOIN, R3D_FACE_DISCON = 1, 2, 4, 8
R3D_INV_NUM = 7
R3D_EV_NAMES = ("generated", "iterations", "scatter", "collect", "catch", "reflect",
                "transfer", "rtsolve", "volume_out")
R3D_EV_NUM = len(R3D_EV_NAMES)
R3D_N_ENERGY, R3D_N_COUNT = 5, 2
R3D_ARRAY_LEGACY, R3D_ARRAY_CURVE = 0, 1   # include/r3d.h r3d_array_image_spec.mode
R3D_N_SCALARS = 3 + R3D_INV_NUM + R3D_EV_NUM

_dp = C.POINTER(C.c_double)


class Face(C.Structure):
    _fields_ = [("normal", C.c_double * 3), ("point", C.c_double * 3), ("radius", C.c_double),
                ("neighbor", C.c_int32), ("flags", C.c_uint32)]


class Cell(C.Structure):
    _fields_ = [("vel_c", C.c_double * 2), ("vel_a", C.c_double * 2),
                ("vel_grad", (C.c_double * 3) * 2), ("rho_c", C.c_double), ("rho_a", C.c_double),
                ("rho_grad", C.c_double * 3), ("q", C.c_double * 2), ("zero_rad2", C.c_double * 2),
                ("scatterer", C.c_int32), ("n_faces", C.c_int32), ("faces", Face * 4)]


class Scatterer(C.Structure):
    _fields_ = [("mfp", C.c_double * 2), ("whole_cdf", (C.c_double * 4) * 2), ("cdf", _dp * 4),
                ("spol", _dp), ("het", C.c_double * 6), ("psdf_numer", C.c_double),
                ("mfp_fixed", C.c_uint32), ("pad_", C.c_uint32)]


class Source(C.Structure):
    _fields_ = [("loc", C.c_double * 3), ("cell", C.c_int32), ("pad_", C.c_int32),
                ("whole_cdf", C.c_double * 3), ("cdf", _dp * 3), ("moment", C.c_double * 6)]


class Seismometer(C.Structure):
    _fields_ = [("loc", C.c_double * 3), ("axes", (C.c_double * 3) * 3), ("r_in", C.c_double * 2),
                ("r_out", C.c_double * 2), ("area", C.c_double * 2)]


class Params(C.Structure):
    _fields_ = [("ttl", C.c_double), ("frequency", C.c_double), ("time_per_bin", C.c_double),
                ("n_bins", C.c_uint32), ("no_deflect", C.c_uint32), ("min_theta", C.c_double),
                ("max_theta", C.c_double), ("slow_concern", C.c_double),
                ("loop_concern", C.c_uint64), ("earth_center", C.c_double * 3)]


class ModelDesc(C.Structure):
    _fields_ = [("cell_kind", C.c_int32), ("n_cells", C.c_int32), ("cells", C.POINTER(Cell)),
                ("n_scatterers", C.c_int32), ("n_seismometers", C.c_int32),
                ("scatterers", C.POINTER(Scatterer)), ("seismometers", C.POINTER(Seismometer)),
                ("n_toa", C.c_uint64), ("toa", _dp), ("source", Source), ("params", Params),
                ("toa_degree", C.c_int32), ("pad_", C.c_int32)]


class GridNode(C.Structure):
    """r3dh_grid_node (include/r3d_host.h): one grid node as the cell builders see it."""
    _fields_ = [("loc", C.c_double * 3), ("radius", C.c_double), ("side", (C.c_double * 9) * 2),
                ("n_sets", C.c_int32), ("pad_", C.c_int32)]


class GridNodeRaw(C.Structure):
    """r3dh_grid_node_raw (include/r3d_host.h): one grid node as the model definition wrote it."""
    _fields_ = [("x", C.c_double * 3), ("set", (C.c_double * 11) * 2), ("n_sets", C.c_int32), ("pad_", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("energy", _dp), ("counts", C.POINTER(C.c_uint64)), ("n_lost", C.c_uint64),
                ("n_timeout", C.c_uint64), ("n_invalid", C.c_uint64),
                ("invalid_reasons", C.c_uint64 * R3D_INV_NUM), ("events", C.c_uint64 * R3D_EV_NUM)]


class VolumeDesc(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("cell_size", C.c_double * 3), ("dims", C.c_uint32 * 3),
                ("n_frames", C.c_uint32), ("frame_dt", C.c_double)]


class VolumeViews(C.Structure):
    """include/r3d.h r3d_volume_views"""
    _fields_ = [("size", C.c_uint32), ("frame_begin", C.c_uint32), ("frame_end", C.c_uint32),
                ("frame_group", C.c_uint32), ("n_range", C.c_uint32), ("pad_", C.c_uint32),
                ("d_range_bin", C.c_void_p), ("d_above", C.c_void_p), ("d_elev", C.c_void_p),
                ("d_outside", C.c_void_p)]


class ViewHeader(C.Structure):
    """include/r3d_host.h r3dh_view_header"""
    _fields_ = [("elevation", C.c_int32), ("dims", C.c_uint32 * 2), ("frames", C.c_uint32), ("group", C.c_uint32),
                ("frame_seconds", C.c_double), ("lo", C.c_double * 2), ("hi", C.c_double * 2), ("dr", C.c_double),
                ("epicentre", C.c_double * 2), ("azimuth", C.c_double), ("half_width", C.c_double),
                ("raw_file", C.c_char_p), ("events_in_view", C.c_uint64), ("events_outside", C.c_uint64)]


class VolumeMaps(C.Structure):
    """include/r3d.h r3d_volume_maps"""
    _fields_ = [("size", C.c_uint32), ("frame_begin", C.c_uint32), ("frame_end", C.c_uint32), ("min_count", C.c_uint32),
                ("d_first", C.c_void_p), ("d_peak_frame", C.c_void_p), ("d_peak_count", C.c_void_p),
                ("d_total", C.c_void_p)]


class WindowSpec(C.Structure):
    """include/r3d.h r3d_window_spec"""
    _fields_ = [("size", C.c_uint32), ("n_seismometers", C.c_uint32), ("n_bins", C.c_uint32), ("n_windows", C.c_uint32),
                ("d_bins", C.c_void_p), ("weight", C.c_double * R3D_N_ENERGY)]


class ArrayImageSpec(C.Structure):
    """include/r3d.h r3d_array_image_spec"""
    _fields_ = [("size", C.c_uint32), ("n_seismometers", C.c_uint32), ("n_bins", C.c_uint32), ("first", C.c_uint32),
                ("last", C.c_uint32), ("gamma_log2", C.c_uint32), ("mode", C.c_int32), ("fit_begin", C.c_uint32),
                ("fit_end", C.c_uint32), ("pad_", C.c_uint32), ("weight", C.c_double * R3D_N_ENERGY), ("rho", C.c_double),
                ("d_curve", C.c_void_p), ("window_length", C.c_double), ("range", C.c_double * 2), ("curve_c", C.c_double),
                ("curve_q", C.c_double)]


class ArrayImageResult(C.Structure):
    """include/r3d.h r3d_array_image_result"""
    _fields_ = [("size", C.c_uint32), ("curve_made", C.c_uint32), ("image", C.c_void_p), ("image_se", C.c_void_p),
                ("summed", C.c_void_p), ("summed_se", C.c_void_p), ("peak", C.c_void_p), ("peak_bin", C.c_void_p),
                ("lit", C.c_void_p), ("batch_row_sum", C.c_void_p), ("fit", C.c_double * 2), ("fit_se", C.c_double * 2),
                ("curve", C.c_void_p), ("image_curve", C.c_void_p), ("image_curve_se", C.c_void_p)]


R3D_ENVELOPE_MAX_SMOOTH, R3D_ENVELOPE_N_SHAPE = 64, 6


class EnvelopeSpec(C.Structure):
    """include/r3d.h r3d_envelope_spec"""
    _fields_ = [("size", C.c_uint32), ("n_seismometers", C.c_uint32), ("n_bins", C.c_uint32), ("first", C.c_uint32),
                ("last", C.c_uint32), ("smooth", C.c_uint32), ("pad_", C.c_uint32), ("d_bins", C.c_void_p),
                ("weight", C.c_double * R3D_N_ENERGY)]


class EnvelopeResult(C.Structure):
    """include/r3d.h r3d_envelope_result"""
    _fields_ = [("size", C.c_uint32), ("pad_", C.c_uint32), ("shape", C.c_void_p), ("shape_se", C.c_void_p),
                ("envelope", C.c_void_p), ("envelope_se", C.c_void_p), ("peak_bin", C.c_void_p), ("half_bin", C.c_void_p),
                ("lit", C.c_void_p)]


R3D_BANDS_MAX_REPLICATES = 4096


class BandsSpec(C.Structure):
    """include/r3d.h r3d_bands_spec"""
    _fields_ = [("size", C.c_uint32), ("n_seismometers", C.c_uint32), ("n_bins", C.c_uint32), ("first", C.c_uint32),
                ("last", C.c_uint32), ("smooth", C.c_uint32), ("n_replicates", C.c_uint32), ("tail", C.c_uint32),
                ("d_bins", C.c_void_p), ("seed", C.c_uint64), ("weight", C.c_double * R3D_N_ENERGY)]


class BandsResult(C.Structure):
    """include/r3d.h r3d_bands_result"""
    _fields_ = [("size", C.c_uint32), ("pad_", C.c_uint32), ("envelope", C.c_void_p), ("envelope_lo", C.c_void_p),
                ("envelope_hi", C.c_void_p), ("shape", C.c_void_p), ("shape_lo", C.c_void_p), ("shape_hi", C.c_void_p),
                ("defined", C.c_void_p)]


R3D_MISFIT_N, R3D_MISFIT_MAX_LAG = 6, 64


class MisfitSpec(C.Structure):
    """include/r3d.h r3d_misfit_spec"""
    _fields_ = [("size", C.c_uint32), ("n_seismometers", C.c_uint32), ("n_bins", C.c_uint32), ("first", C.c_uint32),
                ("last", C.c_uint32), ("smooth_syn", C.c_uint32), ("smooth_obs", C.c_uint32), ("max_lag", C.c_uint32),
                ("amplitude", C.c_uint32), ("pad_", C.c_uint32), ("d_bins", C.c_void_p), ("d_observed", C.c_void_p),
                ("weight", C.c_double * R3D_N_ENERGY)]


class MisfitResult(C.Structure):
    """include/r3d.h r3d_misfit_result"""
    _fields_ = [("size", C.c_uint32), ("pad_", C.c_uint32), ("misfit", C.c_void_p), ("misfit_se", C.c_void_p),
                ("xcorr", C.c_void_p), ("xcorr_se", C.c_void_p), ("envelope", C.c_void_p), ("lit", C.c_void_p)]


R3D_SLANT_MAX_SLOWNESS, R3D_SLANT_MAX_WINDOWS, R3D_SLANT_N = 256, 8, 4


class SlantSpec(C.Structure):
    """include/r3d.h r3d_slant_spec"""
    _fields_ = [("size", C.c_uint32), ("n_seismometers", C.c_uint32), ("n_bins", C.c_uint32), ("first", C.c_uint32),
                ("last", C.c_uint32), ("smooth", C.c_uint32), ("amplitude", C.c_uint32), ("n_slowness", C.c_uint32),
                ("n_windows", C.c_uint32), ("pad_", C.c_uint32), ("p0", C.c_double), ("dp", C.c_double),
                ("d_shift_bin", C.c_void_p), ("d_shift_frac", C.c_void_p), ("d_gain", C.c_void_p), ("d_windows", C.c_void_p),
                ("weight", C.c_double * R3D_N_ENERGY)]


class SlantResult(C.Structure):
    """include/r3d.h r3d_slant_result"""
    _fields_ = [("size", C.c_uint32), ("pad_", C.c_uint32), ("stack", C.c_void_p), ("stack_se", C.c_void_p),
                ("fold", C.c_void_p), ("power", C.c_void_p), ("power_se", C.c_void_p), ("picks", C.c_void_p),
                ("picks_se", C.c_void_p)]


R3D_CONTRAST_MAX_WINDOWS, R3D_CONTRAST_MAX_REGIONS, R3D_CONTRAST_N = 8, 8, 3


class ContrastSpec(C.Structure):
    """include/r3d.h r3d_contrast_spec"""
    _fields_ = [("size", C.c_uint32), ("n_seismometers", C.c_uint32), ("n_bins", C.c_uint32), ("first", C.c_uint32),
                ("last", C.c_uint32), ("smooth", C.c_uint32), ("n_windows", C.c_uint32), ("n_regions", C.c_uint32),
                ("regions", (C.c_uint32 * 2) * R3D_CONTRAST_MAX_REGIONS), ("d_bins", C.c_void_p), ("d_gain", C.c_void_p),
                ("weight", C.c_double * R3D_N_ENERGY), ("scale", C.c_double * 2)]


class ContrastResult(C.Structure):
    """include/r3d.h r3d_contrast_result"""
    _fields_ = [("size", C.c_uint32), ("pad_", C.c_uint32), ("contrast", C.c_void_p), ("contrast_se", C.c_void_p),
                ("lit", C.c_void_p), ("window", C.c_void_p), ("window_se", C.c_void_p), ("region", C.c_void_p),
                ("region_se", C.c_void_p), ("region_loo", C.c_void_p)]


R3D_PRECISION_MAX_ROUNDS = 64
R3D_PRECISION_DEFAULT_MASK = 0x18   # P | S: an axis normal to the motion holds rounding noise and would never be met


class PrecisionSpec(C.Structure):
    """include/r3d.h r3d_precision_spec"""
    _fields_ = [("size", C.c_uint32), ("first", C.c_uint32), ("last", C.c_uint32), ("bin_begin", C.c_uint32),
                ("bin_end", C.c_uint32), ("mask", C.c_uint32), ("n_seismometers", C.c_uint32), ("n_bins", C.c_uint32),
                ("min_count", C.c_uint64), ("rel_target", C.c_double), ("coverage", C.c_double)]


class PrecisionReport(C.Structure):
    """include/r3d.h r3d_precision_report"""
    _fields_ = [("size", C.c_uint32), ("rounds", C.c_uint32), ("met", C.c_uint32), ("pad_", C.c_uint32),
                ("histories", C.c_uint64), ("round_histories", C.c_uint64 * R3D_PRECISION_MAX_ROUNDS),
                ("n_selected", C.c_uint64 * R3D_PRECISION_MAX_ROUNDS), ("n_within", C.c_uint64 * R3D_PRECISION_MAX_ROUNDS),
                ("n_zero", C.c_uint64 * R3D_PRECISION_MAX_ROUNDS), ("worst", C.c_double * R3D_PRECISION_MAX_ROUNDS),
                ("per_receiver", C.c_void_p), ("worst_per_receiver", C.c_void_p)]


class TTImageOpts(C.Structure):
    """include/r3d_host.h r3dh_ttimage_opts"""
    _fields_ = [("size", C.c_uint32), ("first", C.c_uint32), ("last", C.c_uint32), ("gamma_log2", C.c_uint32),
                ("fit_begin", C.c_uint32), ("fit_end", C.c_uint32), ("norm", C.c_double), ("axes", C.c_double * 3),
                ("curve_c", C.c_double), ("curve_q", C.c_double)]


class TTImageResult(C.Structure):
    """include/r3d_host.h r3dh_ttimage_result"""
    _fields_ = [("size", C.c_uint32), ("n_batches", C.c_uint32), ("has_fit", C.c_uint32), ("curve_made", C.c_uint32),
                ("distances", C.c_void_p), ("azimuths", C.c_void_p), ("image", C.c_void_p), ("image_se", C.c_void_p),
                ("lit", C.c_void_p), ("summed", C.c_void_p), ("summed_se", C.c_void_p), ("peak", C.c_void_p),
                ("peak_bin", C.c_void_p), ("fit", C.c_double * 2), ("fit_se", C.c_double * 2), ("curve", C.c_void_p),
                ("image_curve", C.c_void_p), ("image_curve_se", C.c_void_p)]


class LapseOpts(C.Structure):
    """include/r3d_host.h r3dh_lapse_opts"""
    _fields_ = [("size", C.c_uint32), ("first", C.c_uint32), ("last", C.c_uint32), ("pad_", C.c_uint32),
                ("phase_edge", C.c_double * 2), ("windows", C.c_double * 4), ("axes", C.c_double * 3),
                ("geospread", C.c_double), ("ranges", C.c_double * 3)]


class LapseResult(C.Structure):
    """include/r3d_host.h r3dh_lapse_result"""
    _fields_ = [("size", C.c_uint32), ("n_batches", C.c_uint32), ("distances", C.c_void_p), ("bins", C.c_void_p),
                ("clipped", C.c_void_p), ("window_energy", C.c_void_p), ("window_se", C.c_void_p),
                ("window_counts", C.c_void_p), ("batch_window_energy", C.c_void_p)]


class EnvBandsOpts(C.Structure):
    """include/r3d_host.h r3dh_envbands_opts"""
    _fields_ = [("size", C.c_uint32), ("first", C.c_uint32), ("last", C.c_uint32), ("smooth", C.c_uint32),
                ("n_replicates", C.c_uint32), ("tail", C.c_uint32), ("seed", C.c_uint64), ("level", C.c_double),
                ("phase_edge", C.c_double * 2), ("window", C.c_double * 2), ("axes", C.c_double * 3)]


class EnvBandsResult(C.Structure):
    """include/r3d_host.h r3dh_envbands_result"""
    _fields_ = [("size", C.c_uint32), ("n_batches", C.c_uint32), ("distances", C.c_void_p), ("bins", C.c_void_p),
                ("clipped", C.c_void_p), ("envelope", C.c_void_p), ("envelope_lo", C.c_void_p), ("envelope_hi", C.c_void_p),
                ("shape", C.c_void_p), ("shape_lo", C.c_void_p), ("shape_hi", C.c_void_p), ("defined", C.c_void_p)]


class EnvShapeOpts(C.Structure):
    """include/r3d_host.h r3dh_envshape_opts"""
    _fields_ = [("size", C.c_uint32), ("first", C.c_uint32), ("last", C.c_uint32), ("smooth", C.c_uint32),
                ("phase_edge", C.c_double * 2), ("window", C.c_double * 2), ("axes", C.c_double * 3)]


class SlantOpts(C.Structure):
    """include/r3d_host.h r3dh_slant_opts"""
    _fields_ = [("size", C.c_uint32), ("first", C.c_uint32), ("last", C.c_uint32), ("smooth", C.c_uint32),
                ("amplitude", C.c_uint32), ("n_slowness", C.c_uint32), ("n_windows", C.c_uint32), ("pad_", C.c_uint32),
                ("p_min", C.c_double), ("p_max", C.c_double), ("r_ref", C.c_double), ("range_power", C.c_double),
                ("axes", C.c_double * 3), ("windows", (C.c_double * 2) * 8)]


class ContrastOpts(C.Structure):
    """include/r3d_host.h r3dh_contrast_opts"""
    _fields_ = [("size", C.c_uint32), ("first", C.c_uint32), ("last", C.c_uint32), ("smooth", C.c_uint32),
                ("n_windows", C.c_uint32), ("n_regions", C.c_uint32), ("n_test_args", C.c_uint32), ("pad_", C.c_uint32),
                ("seed", C.c_uint64), ("num_phonons", C.c_uint64), ("range_power", C.c_double), ("axes", C.c_double * 3),
                ("velocities", (C.c_double * 2) * 8), ("regions", (C.c_double * 2) * 8), ("test_args", C.POINTER(C.c_double))]


class EnvShapeResult(C.Structure):
    """include/r3d_host.h r3dh_envshape_result"""
    _fields_ = [("size", C.c_uint32), ("n_batches", C.c_uint32), ("distances", C.c_void_p), ("bins", C.c_void_p),
                ("clipped", C.c_void_p), ("shape", C.c_void_p), ("shape_se", C.c_void_p), ("envelope", C.c_void_p),
                ("envelope_se", C.c_void_p), ("peak_bin", C.c_void_p), ("half_bin", C.c_void_p), ("lit", C.c_void_p)]


class EnvFitOpts(C.Structure):
    """include/r3d_host.h r3dh_envfit_opts"""
    _fields_ = [("size", C.c_uint32), ("first", C.c_uint32), ("last", C.c_uint32), ("smooth_syn", C.c_uint32),
                ("smooth_obs", C.c_uint32), ("amplitude", C.c_uint32), ("energy_file", C.c_uint32), ("pad_", C.c_uint32),
                ("phase_edge", C.c_double * 2), ("window", C.c_double * 2), ("axes", C.c_double * 3),
                ("max_lag_seconds", C.c_double), ("file", C.c_char_p)]


class EnvFitResult(C.Structure):
    """include/r3d_host.h r3dh_envfit_result"""
    _fields_ = [("size", C.c_uint32), ("n_batches", C.c_uint32), ("max_lag", C.c_uint32), ("pad_", C.c_uint32),
                ("distances", C.c_void_p), ("bins", C.c_void_p), ("clipped", C.c_void_p), ("observed", C.c_void_p),
                ("misfit", C.c_void_p), ("misfit_se", C.c_void_p), ("xcorr", C.c_void_p), ("xcorr_se", C.c_void_p),
                ("envelope", C.c_void_p), ("lit", C.c_void_p)]


class MapsHeader(C.Structure):
    """include/r3d_host.h r3dh_maps_header"""
    _fields_ = [("dims", C.c_uint32 * 3), ("frames", C.c_uint32), ("min_count", C.c_uint32), ("n_range", C.c_uint32),
                ("frame_seconds", C.c_double), ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("dr", C.c_double),
                ("epicentre", C.c_double * 2), ("azimuth", C.c_double), ("half_width", C.c_double),
                ("prefix", C.c_char_p)]


class Final(C.Structure):
    _fields_ = [("time", C.c_double), ("path", C.c_double), ("amp", C.c_double),
                ("loc", C.c_double * 3), ("dir", C.c_double * 3), ("moves", C.c_uint32),
                ("fate", C.c_uint8), ("type", C.c_uint8), ("n_catch", C.c_uint16)]


class Event(C.Structure):
    """r3d_event (include/r3d.h): one report-stream record."""
    _fields_ = [("id", C.c_uint64), ("time", C.c_double), ("path", C.c_double), ("amp", C.c_double),
                ("loc", C.c_double * 3), ("dir", C.c_double * 3), ("cell", C.c_uint32),
                ("moves", C.c_uint32), ("tag", C.c_uint8), ("type", C.c_uint8), ("pad_", C.c_uint8 * 6)]


R3D_RPT_TAGS = ("GEN", "SCT", "REF", "COL", "CEL", "LST", "TMO", "INV")
R3D_RPT_ALL = 255


def event_dtype():
    """numpy view of an r3d_event array."""
    import numpy as np
    return np.dtype([("id", "<u8"), ("time", "<f8"), ("path", "<f8"), ("amp", "<f8"), ("loc", "<f8", 3),
                     ("dir", "<f8", 3), ("cell", "<u4"), ("moves", "<u4"), ("tag", "u1"), ("type", "u1"),
                     ("pad_", "u1", 6)])


def _load(path):
    if not os.path.exists(path):
        raise RuntimeError(
            f"native library missing: {path} -- build it with `make` (or "
            f"`python -c 'import __graft_entry__ as g; g.build()'`); there is no fallback path")
    return C.CDLL(path)


_host = None
_hip = {}


def host_lib():
    """libr3d_host.so: the C++ model builder."""
    global _host
    if _host is None:
        L = _load(os.path.join(LIBDIR, "libr3d_host.so"))
        L.r3dh_model_from_args.restype = C.c_void_p
        L.r3dh_model_from_args.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
        L.r3dh_model_free.argtypes = [C.c_void_p]
        L.r3dh_model_desc.restype = C.POINTER(ModelDesc)
        L.r3dh_model_desc.argtypes = [C.c_void_p]
        L.r3dh_num_phonons.restype = C.c_uint64
        L.r3dh_num_phonons.argtypes = [C.c_void_p]
        L.r3dh_seed.restype = C.c_uint64
        L.r3dh_seed.argtypes = [C.c_void_p]
        L.r3dh_model_log.restype = C.c_char_p
        L.r3dh_model_log.argtypes = [C.c_void_p]
        L.r3dh_grid_dump.restype = C.c_char_p
        L.r3dh_grid_dump.argtypes = [C.c_void_p]
        L.r3dh_scatterer_info.restype = C.c_int
        L.r3dh_scatterer_info.argtypes = [C.c_void_p, C.c_int, _dp]
        L.r3dh_last_error.restype = C.c_char_p
        L.r3dh_scatterer_dump.restype = C.c_char_p
        L.r3dh_scatterer_dump.argtypes = [C.c_void_p]
        L.r3dh_params_echo.restype = C.c_char_p
        L.r3dh_params_echo.argtypes = [C.c_void_p]
        L.r3dh_model_set_scatterer_stats.restype = C.c_int
        L.r3dh_model_set_scatterer_stats.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        L.r3dh_model_device_tables.restype = C.c_int
        L.r3dh_model_device_tables.argtypes = [C.c_void_p]
        L.r3dh_report_mask.restype = C.c_uint32
        L.r3dh_report_mask.argtypes = [C.c_char_p]
        L.r3dh_model_report_mask.restype = C.c_uint32
        L.r3dh_model_report_mask.argtypes = [C.c_void_p]
        L.r3dh_write_reports.restype = C.c_char_p
        L.r3dh_write_reports.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p]
        L.r3dh_write_outputs.restype = C.c_char_p
        L.r3dh_write_outputs.argtypes = [C.c_void_p, C.POINTER(Result), C.c_char_p, C.c_char_p, C.c_char_p]
        L.r3dh_model_coordinates.restype = C.c_int
        L.r3dh_model_coordinates.argtypes = [C.c_void_p, C.POINTER(C.c_int), _dp, C.POINTER(C.c_int)]
        L.r3dh_grid_size.restype = C.c_int
        L.r3dh_grid_size.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.r3dh_grid_nodes.restype = C.c_int
        L.r3dh_grid_nodes.argtypes = [C.c_void_p, C.POINTER(GridNode), C.c_size_t]
        L.r3dh_grid_nodes_raw.restype = C.c_int
        L.r3dh_grid_nodes_raw.argtypes = [C.c_void_p, C.POINTER(GridNodeRaw), C.c_size_t]
        L.r3dh_write_errors.restype = C.c_int
        L.r3dh_write_errors.argtypes = [C.c_void_p, _dp, _dp, C.c_uint32, C.c_char_p]
        L.r3dh_error_batches.restype = C.c_uint32
        L.r3dh_error_batches.argtypes = [C.c_void_p]
        L.r3dh_job_error_batches.restype = C.c_uint32
        L.r3dh_job_error_batches.argtypes = [C.c_void_p]
        L.r3dh_scatter_views.restype = C.c_int
        L.r3dh_scatter_views.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), _dp, C.POINTER(C.c_int)]
        L.r3dh_write_view_header.restype = C.c_int
        L.r3dh_write_view_header.argtypes = [C.POINTER(ViewHeader), C.c_char_p]
        L.r3dh_scatter_maps.restype = C.c_int
        L.r3dh_scatter_maps.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.r3dh_write_maps_header.restype = C.c_int
        L.r3dh_write_maps_header.argtypes = [C.POINTER(MapsHeader), C.c_char_p]
        L.r3dh_lapse_request.restype = C.c_int
        L.r3dh_lapse_request.argtypes = [C.c_void_p, C.POINTER(LapseOpts)]
        L.r3dh_lapse_plan.restype = C.c_int
        L.r3dh_lapse_plan.argtypes = [C.c_void_p, C.POINTER(LapseOpts), _dp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
        L.r3dh_write_lapse.restype = C.c_int
        L.r3dh_write_lapse.argtypes = [C.c_void_p, C.POINTER(LapseOpts), C.POINTER(LapseResult), C.c_char_p]
        L.r3dh_ttimage_request.restype = C.c_int
        L.r3dh_ttimage_request.argtypes = [C.c_void_p, C.POINTER(TTImageOpts)]
        L.r3dh_ttimage_plan.restype = C.c_int
        L.r3dh_ttimage_plan.argtypes = [C.c_void_p, C.POINTER(TTImageOpts), _dp, _dp]
        L.r3dh_write_ttimage.restype = C.c_int
        L.r3dh_write_ttimage.argtypes = [C.c_void_p, C.POINTER(TTImageOpts), C.POINTER(TTImageResult), C.c_char_p]
        L.r3dh_envshape_request.restype = C.c_int
        L.r3dh_envshape_request.argtypes = [C.c_void_p, C.POINTER(EnvShapeOpts)]
        L.r3dh_envshape_plan.restype = C.c_int
        L.r3dh_envshape_plan.argtypes = [C.c_void_p, C.POINTER(EnvShapeOpts), _dp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
        L.r3dh_write_envshape.restype = C.c_int
        L.r3dh_write_envshape.argtypes = [C.c_void_p, C.POINTER(EnvShapeOpts), C.POINTER(EnvShapeResult), C.c_char_p]
        L.r3dh_envbands_request.restype = C.c_int
        L.r3dh_envbands_request.argtypes = [C.c_void_p, C.POINTER(EnvBandsOpts)]
        L.r3dh_envbands_plan.restype = C.c_int
        L.r3dh_envbands_plan.argtypes = [C.c_void_p, C.POINTER(EnvBandsOpts), _dp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
        L.r3dh_write_envbands.restype = C.c_int
        L.r3dh_write_envbands.argtypes = [C.c_void_p, C.POINTER(EnvBandsOpts), C.POINTER(EnvBandsResult), C.c_char_p]
        L.r3dh_slant_request.restype = C.c_int
        L.r3dh_slant_request.argtypes = [C.c_void_p, C.POINTER(SlantOpts)]
        L.r3dh_slant_plan.restype = C.c_int
        L.r3dh_slant_plan.argtypes = [C.c_void_p, C.POINTER(SlantOpts), _dp, _dp, C.POINTER(C.c_int32), _dp, _dp,
                                      C.POINTER(C.c_uint32)]
        L.r3dh_contrast_request.restype = C.c_int
        L.r3dh_contrast_request.argtypes = [C.c_void_p, C.POINTER(ContrastOpts)]
        L.r3dh_contrast_plan.restype = C.c_int
        L.r3dh_contrast_plan.argtypes = [C.c_void_p, C.POINTER(ContrastOpts), _dp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_uint32), _dp, _dp]
        L.r3dh_observed_to_bins.restype = C.c_int
        L.r3dh_observed_to_bins.argtypes = [_dp, C.c_uint32, C.c_uint32] + [C.c_double] * 4 + [C.c_uint32, _dp]
        L.r3dh_read_octave.restype = C.c_int
        L.r3dh_read_octave.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _dp, C.c_size_t]
        L.r3dh_envfit_request.restype = C.c_int
        L.r3dh_envfit_request.argtypes = [C.c_void_p, C.POINTER(EnvFitOpts)]
        L.r3dh_envfit_plan.restype = C.c_int
        L.r3dh_envfit_plan.argtypes = [C.c_void_p, C.POINTER(EnvFitOpts), _dp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), _dp,
                                       C.POINTER(C.c_uint32)]
        L.r3dh_write_envfit.restype = C.c_int
        L.r3dh_write_envfit.argtypes = [C.c_void_p, C.POINTER(EnvFitOpts), C.POINTER(EnvFitResult), C.c_char_p]
        L.r3dh_precision_request.restype = C.c_int
        L.r3dh_precision_request.argtypes = [C.c_void_p, C.POINTER(PrecisionSpec), C.POINTER(C.c_uint32)]
        L.r3dh_write_precision.restype = C.c_int
        L.r3dh_write_precision.argtypes = [C.POINTER(PrecisionSpec), C.c_uint32, C.c_uint32, C.c_uint64,
                                           C.POINTER(PrecisionReport), C.c_char_p]
        L.r3dh_seismometer_axes.restype = C.c_int
        L.r3dh_seismometer_axes.argtypes = [C.c_void_p, C.c_int]
        _host = L
    return _host


R3D_COMM_ID_BYTES = 128


class CommInfo(C.Structure):   # include/r3d.h r3d_comm_info
    _fields_ = [("n_ranks", C.c_int32), ("rank", C.c_int32), ("device", C.c_int32), ("rccl_version", C.c_int32),
                ("device_uuid", C.c_char * 40), ("library", C.c_char * 256)]


class EngineOpts(C.Structure):
    """include/r3d.h r3d_engine_opts"""
    _fields_ = [("size", C.c_uint32), ("residency", C.c_int32), ("pool_slots", C.c_uint32),
                ("accumulator_bits", C.c_int32), ("lds_reserve", C.c_uint32)]


def hip_lib(reproducible=False, path=None):
    """libr3d_hip.so: the HIP engine.  Fails loudly when it was not built.

    reproducible: libr3d_hip_repro.so, the same engine built with -DR3D_REPRODUCIBLE -- no
    wave-voted series choices (csrc/r3d_math.h all_lanes), so a history's result is bit-defined by
    (model, seed, id).  path: another build of the engine (a `make variant` library, tools/); nothing
    here or in the library reads the environment."""
    key = os.path.abspath(path) if path else bool(reproducible)
    if key not in _hip:
        # One HIP runtime per process: torch ships its own libamdhip64, and whichever copy is loaded first
        # serves everyone (same SONAME).  The harness allocates result blocks and grids as torch tensors, so
        # torch's copy has to be that one -- loaded the other way round, torch finds "no HIP GPUs".
        import torch  # noqa: F401
        L = _load(path or os.path.join(LIBDIR, "libr3d_hip_repro.so" if reproducible else "libr3d_hip.so"))
        L.r3d_engine_create.restype = C.c_void_p
        L.r3d_engine_create.argtypes = [C.POINTER(ModelDesc), C.c_int]
        L.r3d_engine_create_ex.restype = C.c_void_p
        L.r3d_engine_create_ex.argtypes = [C.POINTER(ModelDesc), C.c_int, C.POINTER(EngineOpts)]
        L.r3d_engine_destroy.argtypes = [C.c_void_p]
        L.r3d_energy_len.restype = C.c_size_t
        L.r3d_energy_len.argtypes = [C.c_void_p]
        L.r3d_counts_len.restype = C.c_size_t
        L.r3d_counts_len.argtypes = [C.c_void_p]
        L.r3d_run.restype = C.c_int
        L.r3d_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(Result)]
        L.r3d_run_traced.restype = C.c_int
        L.r3d_run_traced.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                     C.POINTER(Result), C.POINTER(Final)]
        L.r3d_run_device.restype = C.c_int
        L.r3d_run_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.r3d_engine_set_volume.restype = C.c_int
        L.r3d_engine_set_volume.argtypes = [C.c_void_p, C.POINTER(VolumeDesc)]
        L.r3d_volume_len.restype = C.c_size_t
        L.r3d_volume_len.argtypes = [C.c_void_p]
        L.r3d_volume_read.restype = C.c_int
        L.r3d_volume_read.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int]
        L.r3d_volume_device_ptr.restype = C.c_void_p
        L.r3d_volume_device_ptr.argtypes = [C.c_void_p]
        L.r3d_run_device_carry.restype = C.c_int
        L.r3d_run_device_carry.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.r3d_run_model.restype = C.c_int
        L.r3d_run_model.argtypes = [C.POINTER(ModelDesc), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int,
                                    C.POINTER(Result)]
        L.r3d_engine_scatterer_stats.restype = C.c_int
        L.r3d_engine_scatterer_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.r3d_engine_download_scatterer.restype = C.c_int
        L.r3d_engine_download_scatterer.argtypes = [C.c_void_p, C.c_int, C.POINTER(_dp), _dp]
        L.r3d_engine_download_source.restype = C.c_int
        L.r3d_engine_download_source.argtypes = [C.c_void_p, C.POINTER(_dp), _dp]
        L.r3d_engine_download_toa.restype = C.c_int
        L.r3d_engine_download_toa.argtypes = [C.c_void_p, _dp]
        L.r3d_engine_set_event_log.restype = C.c_int
        L.r3d_engine_set_event_log.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
        L.r3d_event_log_count.restype = C.c_uint64
        L.r3d_event_log_count.argtypes = [C.c_void_p]
        L.r3d_event_log_read.restype = C.c_uint64
        L.r3d_event_log_read.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        L.r3d_last_kernel_ms.restype = C.c_double
        L.r3d_last_kernel_ms.argtypes = [C.c_void_p]
        L.r3d_launch_count.restype = C.c_uint64
        L.r3d_launch_count.argtypes = [C.c_void_p]
        L.r3d_selftest_math.restype = C.c_int
        L.r3d_selftest_math.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.c_uint64]
        L.r3d_kernel_ms.restype = C.c_double
        L.r3d_kernel_ms.argtypes = [C.c_void_p, C.c_uint64]
        L.r3d_engine_close.restype = C.c_int
        L.r3d_engine_close.argtypes = [C.c_void_p]
        L.r3d_engine_carry_pending.restype = C.c_int
        L.r3d_engine_carry_pending.argtypes = [C.c_void_p]
        L.r3d_engine_set_volume_buffer.restype = C.c_int
        L.r3d_engine_set_volume_buffer.argtypes = [C.c_void_p, C.POINTER(VolumeDesc), C.c_void_p]
        L.r3d_engine_set_production_finals.restype = C.c_int
        L.r3d_engine_set_production_finals.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
        L.r3d_production_finals_read.restype = C.c_int
        L.r3d_production_finals_read.argtypes = [C.c_void_p, C.POINTER(Final), C.c_uint64, C.c_uint64]
        L.r3d_node_create.restype = C.c_void_p
        L.r3d_node_create.argtypes = [C.POINTER(ModelDesc), C.POINTER(C.c_int), C.c_int]
        L.r3d_node_run.restype = C.c_int
        L.r3d_node_run.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(Result)]
        L.r3d_node_size.restype = C.c_int
        L.r3d_node_size.argtypes = [C.c_void_p]
        L.r3d_node_engine.restype = C.c_void_p
        L.r3d_node_engine.argtypes = [C.c_void_p, C.c_int]
        L.r3d_node_reduction.restype = C.c_char_p
        L.r3d_node_reduction.argtypes = [C.c_void_p]
        L.r3d_node_reduction_note.restype = C.c_char_p
        L.r3d_node_reduction_note.argtypes = [C.c_void_p]
        L.r3d_node_destroy.argtypes = [C.c_void_p]
        L.r3d_comm_unique_id.restype = C.c_int
        L.r3d_comm_unique_id.argtypes = [C.c_char_p]
        L.r3d_comm_create.restype = C.c_void_p
        L.r3d_comm_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int]
        L.r3d_comm_reduce.restype = C.c_int
        L.r3d_comm_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                      C.c_int, C.c_void_p]
        L.r3d_comm_describe.restype = C.c_int
        L.r3d_comm_describe.argtypes = [C.c_void_p, C.POINTER(CommInfo)]
        L.r3d_comm_destroy.argtypes = [C.c_void_p]
        L.r3d_run_model_on.restype = C.c_int
        L.r3d_run_model_on.argtypes = [C.POINTER(ModelDesc), C.c_uint64, C.c_uint64, C.c_uint64,
                                       C.POINTER(C.c_int), C.c_int, C.POINTER(Result)]
        L.r3d_engine_variant.restype = C.c_int
        L.r3d_engine_variant.argtypes = [C.c_void_p]
        L.r3d_engine_accumulators.restype = C.c_uint32
        L.r3d_engine_accumulators.argtypes = [C.c_void_p]
        L.r3d_engine_pool_slots.restype = C.c_uint32
        L.r3d_engine_pool_slots.argtypes = [C.c_void_p]
        L.r3d_volume_compact.restype = C.c_int
        L.r3d_volume_compact.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.c_void_p]
        L.r3d_volume_scatter_add.restype = C.c_int
        L.r3d_volume_scatter_add.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                             C.c_void_p]
        L.r3d_volume_read_range.restype = C.c_int
        L.r3d_volume_read_range.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
        L.r3d_volume_reduce_by_frame.restype = C.c_int
        L.r3d_volume_reduce_by_frame.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        L.r3d_volume_project.restype = C.c_int
        L.r3d_volume_project.argtypes = [C.c_int, C.c_void_p, C.POINTER(VolumeDesc), C.POINTER(VolumeViews), C.c_void_p]
        L.r3d_volume_range_bins.restype = C.c_int
        L.r3d_volume_range_bins.argtypes = [C.POINTER(VolumeDesc), _dp, C.c_double, C.c_uint32, C.c_double, C.c_double,
                                            C.POINTER(C.c_uint32)]
        L.r3d_volume_project_to_host.restype = C.c_int
        L.r3d_volume_project_to_host.argtypes = [C.c_int, C.c_void_p, C.POINTER(VolumeDesc), C.c_uint32, C.c_uint32, C.c_uint32,
                                                 C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
        L.r3d_volume_time_maps.restype = C.c_int
        L.r3d_volume_time_maps.argtypes = [C.c_int, C.c_void_p, C.POINTER(VolumeDesc), C.POINTER(VolumeMaps), C.c_void_p]
        L.r3d_volume_time_maps_to_host.restype = C.c_int
        L.r3d_volume_time_maps_to_host.argtypes = [C.c_int, C.c_void_p, C.POINTER(VolumeDesc), C.c_uint32, C.c_uint32, C.c_uint32,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.r3d_batch_moments.restype = C.c_int
        L.r3d_batch_moments.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                        C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.r3d_run_device_batched.restype = C.c_int
        L.r3d_run_device_batched.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]
        L.r3d_run_batched.restype = C.c_int
        L.r3d_run_batched.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(Result),
                                      _dp, _dp]
        L.r3d_batch_partial.restype = C.c_int
        L.r3d_batch_partial.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                        C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.r3d_batch_merge.restype = C.c_int
        L.r3d_batch_merge.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                      C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
        L.r3d_node_run_batched.restype = C.c_int
        L.r3d_node_run_batched.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(Result),
                                           _dp, _dp]
        L.r3d_window_sums.restype = C.c_int
        L.r3d_window_sums.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(WindowSpec), C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
        L.r3d_window_bins.restype = C.c_int
        L.r3d_window_bins.argtypes = [C.c_double, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.r3d_window_log_ratio.restype = C.c_int
        L.r3d_window_log_ratio.argtypes = [C.c_uint32, _dp, _dp, C.c_uint64, _dp, _dp]
        L.r3d_array_image.restype = C.c_int
        L.r3d_array_image.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.POINTER(ArrayImageSpec)] + [C.c_void_p] * 8
        L.r3d_array_powerlaw.restype = C.c_int
        L.r3d_array_powerlaw.argtypes = [C.c_uint32, C.c_double, C.c_double, _dp, C.c_uint64, C.c_uint32, C.c_uint32, _dp]
        L.r3d_array_powerlaw_jackknife.restype = C.c_int
        L.r3d_array_powerlaw_jackknife.argtypes = [C.c_uint32, C.c_double, C.c_double, C.c_uint32, _dp, C.c_uint64, C.c_uint32,
                                                   C.c_uint32, _dp, _dp, _dp]
        L.r3d_run_batched_array_image.restype = C.c_int
        L.r3d_run_batched_array_image.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(Result),
                                                  _dp, _dp, C.POINTER(ArrayImageSpec), C.POINTER(ArrayImageResult)]
        L.r3d_envelope_shape.restype = C.c_int
        L.r3d_envelope_shape.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.POINTER(EnvelopeSpec)] + [C.c_void_p] * 9
        L.r3d_run_batched_envelope_shape.restype = C.c_int
        L.r3d_run_batched_envelope_shape.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                                     C.POINTER(Result), _dp, _dp, C.POINTER(EnvelopeSpec),
                                                     C.POINTER(EnvelopeResult)]
        L.r3d_bootstrap_counts.restype = C.c_int
        L.r3d_bootstrap_counts.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
        L.r3d_bootstrap_counts_device.restype = C.c_int
        L.r3d_bootstrap_counts_device.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.r3d_envelope_bands.restype = C.c_int
        L.r3d_envelope_bands.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.POINTER(BandsSpec)] + [C.c_void_p] * 9
        L.r3d_run_batched_envelope_bands.restype = C.c_int
        L.r3d_run_batched_envelope_bands.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                                     C.POINTER(Result), _dp, _dp, C.POINTER(BandsSpec),
                                                     C.POINTER(BandsResult)]
        L.r3d_envelope_misfit.restype = C.c_int
        L.r3d_envelope_misfit.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.POINTER(MisfitSpec)] + [C.c_void_p] * 9
        L.r3d_run_batched_envelope_misfit.restype = C.c_int
        L.r3d_run_batched_envelope_misfit.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                                      C.POINTER(Result), _dp, _dp, C.POINTER(MisfitSpec),
                                                      C.POINTER(MisfitResult)]
        L.r3d_slant_shifts.restype = C.c_int
        L.r3d_slant_shifts.argtypes = [C.c_double, C.c_uint32, _dp, C.c_double, C.c_double, C.c_double, C.c_uint32,
                                       C.POINTER(C.c_int32), _dp]
        L.r3d_slant_stack.restype = C.c_int
        L.r3d_slant_stack.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.POINTER(SlantSpec)] + [C.c_void_p] * 10
        L.r3d_run_batched_slant_stack.restype = C.c_int
        L.r3d_run_batched_slant_stack.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                                  C.POINTER(Result), _dp, _dp, C.POINTER(SlantSpec), C.POINTER(SlantResult)]
        L.r3d_contrast_decibel.restype = C.c_int
        L.r3d_contrast_decibel.argtypes = [C.c_uint32, C.c_uint32, C.c_double, _dp, _dp, _dp]
        L.r3d_contrast_gains.restype = C.c_int
        L.r3d_contrast_gains.argtypes = [C.c_uint32, _dp, C.c_double, C.c_double, _dp]
        L.r3d_array_contrast.restype = C.c_int
        L.r3d_array_contrast.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(ContrastSpec)] + \
            [C.c_void_p] * 10
        L.r3d_run_batched_contrast.restype = C.c_int
        L.r3d_run_batched_contrast.argtypes = [C.c_void_p, C.c_void_p] + [C.c_uint64] * 5 + [C.c_uint32] * 2 + \
            [C.POINTER(Result)] * 2 + [_dp] * 4 + [C.POINTER(ContrastSpec), C.POINTER(ContrastResult)]
        L.r3d_run_batched_windows.restype = C.c_int
        L.r3d_run_batched_windows.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(Result),
                                              _dp, _dp, C.POINTER(WindowSpec), _dp, C.POINTER(C.c_uint64), _dp, _dp]
        L.r3d_batch_precision.restype = C.c_int
        L.r3d_batch_precision.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                          C.POINTER(PrecisionSpec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.r3d_run_to_precision.restype = C.c_int
        L.r3d_run_to_precision.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                           C.POINTER(PrecisionSpec), C.POINTER(Result), _dp, _dp, C.POINTER(PrecisionReport)]
        L.r3d_last_error.restype = C.c_char_p
        L.r3d_version.restype = C.c_char_p
        _hip[key] = L
    return _hip[key]
