"""Host-side Python mirror of the reference's run interface for the hot path.

``Model(args)`` takes the reference's own command-line tokens (the ones a
do-*.sh script assembles, scripts/do-fundamentals.sh:396-419) and builds the
flat tables through the C++ builder (libr3d_host.so).  ``Engine(model)`` puts
them in HBM and ``Engine.run(n, first_id, seed)`` is the drop-in for the body
of ``Model::RunSimulation()`` (reference model.cpp:602-633): N histories of
GenerateEventPhonon + Propagate, returning filled seismometer bins and the
loss counters.

There is no CPU fallback here: without libr3d_hip.so (or without a GPU)
``Engine`` raises.
"""
import ctypes as C
import math

import numpy as np

from . import _ffi


class Result:
    """Seismometer bins + counters of a run (reference BinRecord,
    dataout.hpp:77-93, and DataReporter counters, dataout.cpp:591-617)."""

    def __init__(self, n_seis, n_bins):
        self.n_seis, self.n_bins = n_seis, n_bins
        self.energy = np.zeros((n_seis, n_bins, _ffi.R3D_N_ENERGY), dtype=np.float64)
        self.counts = np.zeros((n_seis, n_bins, _ffi.R3D_N_COUNT), dtype=np.uint64)
        self.n_lost = self.n_timeout = self.n_invalid = 0
        self.invalid_reasons = np.zeros(_ffi.R3D_INV_NUM, dtype=np.uint64)
        self.events = dict.fromkeys(_ffi.R3D_EV_NAMES, 0)

    # -- C view -------------------------------------------------------------
    def _as_c(self):
        r = _ffi.Result()
        r.energy = self.energy.ctypes.data_as(C.POINTER(C.c_double))
        r.counts = self.counts.ctypes.data_as(C.POINTER(C.c_uint64))
        r.n_lost, r.n_timeout, r.n_invalid = self.n_lost, self.n_timeout, self.n_invalid
        for i in range(_ffi.R3D_INV_NUM):
            r.invalid_reasons[i] = int(self.invalid_reasons[i])
        for i, k in enumerate(_ffi.R3D_EV_NAMES):
            r.events[i] = self.events[k]
        return r

    def _from_c(self, r):
        self.n_lost, self.n_timeout, self.n_invalid = int(r.n_lost), int(r.n_timeout), int(r.n_invalid)
        for i in range(_ffi.R3D_INV_NUM):
            self.invalid_reasons[i] = r.invalid_reasons[i]
        for i, k in enumerate(_ffi.R3D_EV_NAMES):
            self.events[k] = int(r.events[i])

    @property
    def diag_invalid(self):
        """7-bit OR of the invalid reasons (DataReporter::mDiagInvalid)."""
        return sum(1 << i for i in range(_ffi.R3D_INV_NUM) if self.invalid_reasons[i])

    def scalars(self):
        return np.array([self.n_lost, self.n_timeout, self.n_invalid, *self.invalid_reasons,
                         *[self.events[k] for k in _ffi.R3D_EV_NAMES]], dtype=np.uint64)

    def set_scalars(self, v):
        v = [int(x) for x in v]
        self.n_lost, self.n_timeout, self.n_invalid = v[0:3]
        self.invalid_reasons[:] = v[3:3 + _ffi.R3D_INV_NUM]
        for i, k in enumerate(_ffi.R3D_EV_NAMES):
            self.events[k] = v[3 + _ffi.R3D_INV_NUM + i]


class Model:
    """A built, immutable Earth model + source + seismometers."""

    def __init__(self, args):
        if isinstance(args, str):
            args = args.split()
        self._lib = _ffi.host_lib()
        self.args = list(args)
        argv = (C.c_char_p * len(args))(*[a.encode() for a in args])
        self._h = self._lib.r3dh_model_from_args(len(args), argv)
        if not self._h:
            raise RuntimeError("model build failed: " + self._lib.r3dh_last_error().decode())
        self.desc_p = self._lib.r3dh_model_desc(self._h)
        self.desc = self.desc_p.contents

    def close(self):
        if getattr(self, "_h", None):
            self._lib.r3dh_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- facts about the model ------------------------------------------------
    @property
    def n_cells(self):
        return self.desc.n_cells

    @property
    def n_scatterers(self):
        return self.desc.n_scatterers

    @property
    def n_seismometers(self):
        return self.desc.n_seismometers

    @property
    def n_bins(self):
        return self.desc.params.n_bins

    @property
    def n_toa(self):
        return self.desc.n_toa

    @property
    def num_phonons(self):
        return int(self._lib.r3dh_num_phonons(self._h))

    @property
    def seed(self):
        return int(self._lib.r3dh_seed(self._h))

    @property
    def log(self):
        return self._lib.r3dh_model_log(self._h).decode()

    def grid_dump(self):
        return self._lib.r3dh_grid_dump(self._h).decode()

    def scatterer_info(self, i):
        out = (C.c_double * 10)()
        if self._lib.r3dh_scatterer_info(self._h, i, out):
            raise IndexError(i)
        keys = ("nu", "eps", "a", "kappa", "el", "gam0", "mfp_p", "mfp_s", "dipole_p", "dipole_s")
        return dict(zip(keys, out))

    def scatterer_dump(self):
        return self._lib.r3dh_scatterer_dump(self._h).decode()

    def params_echo(self):
        return self._lib.r3dh_params_echo(self._h).decode()

    def write_outputs(self, result, outdir, trace_path=None, mparams_path=None):
        """Write seis_NNN.octv (+ ASCII traces, + parameter file) in the reference's
        formats; returns the post-sim console summary."""
        import os
        trace_path = trace_path or os.path.join(outdir or ".", "seis_traces_asc.dat")
        c = result._as_c()
        txt = self._lib.r3dh_write_outputs(self._h, C.byref(c), (outdir or "").encode(), trace_path.encode(),
                                           mparams_path.encode() if mparams_path else None)
        if txt is None:
            raise RuntimeError("write_outputs failed: " + self._lib.r3dh_last_error().decode())
        return txt.decode()

    @property
    def coordinates(self):
        """(map code, Earth radius, flattened) of the coordinate system the model was built in
        (reference ecs.hpp:242-257: 0 ENU_ORTHO, 1 RAE_ORTHO, 2 RAE_CURVED, 3 RAE_SPHERICAL)."""
        code, flat, rad = C.c_int(), C.c_int(), C.c_double()
        self._lib.r3dh_model_coordinates(self._h, C.byref(code), C.byref(rad), C.byref(flat))
        return code.value, rad.value, bool(flat.value)

    def grid_nodes(self):
        """((ni, nj, nk), array of _ffi.GridNode): the grid as the cell builders see it.  Call right
        after building the model (the coordinate system is process-global, as in the reference)."""
        dims = (C.c_int * 3)()
        self._lib.r3dh_grid_size(self._h, dims)
        n = dims[0] * dims[1] * dims[2]
        nodes = (_ffi.GridNode * n)()
        if self._lib.r3dh_grid_nodes(self._h, nodes, n):
            raise RuntimeError("r3dh_grid_nodes failed: " + self._lib.r3dh_last_error().decode())
        return tuple(dims), nodes

    def grid_nodes_raw(self):
        """array of _ffi.GridNodeRaw in the grid's own order: the nodes before the coordinate system's conversion."""
        dims = (C.c_int * 3)()
        self._lib.r3dh_grid_size(self._h, dims)
        n = dims[0] * dims[1] * dims[2]
        nodes = (_ffi.GridNodeRaw * n)()
        if self._lib.r3dh_grid_nodes_raw(self._h, nodes, n):
            raise RuntimeError("r3dh_grid_nodes_raw failed: " + self._lib.r3dh_last_error().decode())
        return nodes

    def seismometer_axes(self, i):
        """0 ENZ, 1 RTZ (model.cpp:486-491)."""
        return int(self._lib.r3dh_seismometer_axes(self._h, i))

    @property
    def device_tables(self):
        """True if built with --device-tables: the scattering tables are made by the engine."""
        return bool(self._lib.r3dh_model_device_tables(self._h))

    @property
    def report_mask(self):
        """R3D_RPT_* mask asked for by --reports in the model's arguments."""
        return int(self._lib.r3dh_model_report_mask(self._h))

    def format_reports(self, events, path=None):
        """Event records (Engine.read_event_log) as the reference's report lines
        (dataout.cpp:484-520); written to `path`, or returned as text."""
        import numpy as np
        ev = np.ascontiguousarray(events, dtype=_ffi.event_dtype())
        txt = self._lib.r3dh_write_reports(self._h, ev.ctypes.data, len(ev), path.encode() if path else None)
        if txt is None:
            raise RuntimeError("write_reports failed: " + self._lib.r3dh_last_error().decode())
        return txt.decode()

    def write_errors(self, energy_se, counts_se, n_batches, outdir):
        """Write seis_NNN_err.octv beside each seis_NNN.octv: the standard errors of a batched run
        (Engine.run_batched) as matrices TraceXYZ_se, TracePS_se, CountPS_se and the scalar NumBatches."""
        shape = (self.n_seismometers, self.n_bins)
        e = np.ascontiguousarray(energy_se, dtype=np.float64).reshape(shape + (_ffi.R3D_N_ENERGY,))
        c = np.ascontiguousarray(counts_se, dtype=np.float64).reshape(shape + (_ffi.R3D_N_COUNT,))
        if self._lib.r3dh_write_errors(self._h, e.ctypes.data_as(_ffi._dp), c.ctypes.data_as(_ffi._dp), int(n_batches),
                                       (outdir or "").encode()):
            raise RuntimeError("write_errors failed: " + self._lib.r3dh_last_error().decode())

    @property
    def error_batches(self):
        """What --error-batches=B in the model's arguments asked for (0: absent)."""
        return int(self._lib.r3dh_error_batches(self._h))

    @property
    def job_error_batches(self):
        """What --job-error-batches=N in the model's arguments asked for: the batches of the whole job, over whatever
        shards --gpus / --devices name (0: absent)."""
        return int(self._lib.r3dh_job_error_batches(self._h))

    @property
    def scatter_views(self):
        """What --scatter-views[=GROUP] [--scatter-view-azimuth=AZI,HALFWIDTH] [--no-scatter-grid-file] asked for:
        None, or dict(group, azimuth, half_width, no_grid_file)."""
        group, azi, no_file = C.c_uint32(0), (C.c_double * 2)(), C.c_int(0)
        if not self._lib.r3dh_scatter_views(self._h, C.byref(group), azi, C.byref(no_file)):
            return None
        return dict(group=int(group.value), azimuth=azi[0], half_width=azi[1], no_grid_file=bool(no_file.value))

    @property
    def scatter_maps(self):
        """What --scatter-maps[=MINCOUNT] asked for: None, or the threshold MINCOUNT (default 1)."""
        min_count = C.c_uint32(0)
        if not self._lib.r3dh_scatter_maps(self._h, C.byref(min_count)):
            return None
        return int(min_count.value)

    @property
    def precision_request(self):
        """What --target-error=REL[,COVERAGE[,MINCOUNT[,ROUNDS]]] and its companions (--target-array, --target-components)
        asked for: None, or dict(first, last, mask, min_count, rel, coverage, rounds) -- Engine.run_to_precision's
        arguments of the same names (include/r3d_host.h r3dh_precision_request)."""
        spec, rounds = _ffi.PrecisionSpec(), C.c_uint32(0)
        rc = self._lib.r3dh_precision_request(self._h, C.byref(spec), C.byref(rounds))
        if rc < 0:
            raise RuntimeError("precision_request failed: " + self._lib.r3dh_last_error().decode())
        if rc == 0:
            return None
        return dict(first=int(spec.first), last=int(spec.last), mask=int(spec.mask), min_count=int(spec.min_count),
                    rel=spec.rel_target, coverage=spec.coverage, rounds=int(rounds.value))

    @property
    def lapse_request(self):
        """What --lapse-windows[=V,T0,B1,E1,B2,E2] and its companions (--lapse-axes, --lapse-geospread, --lapse-ranges,
        --lapse-array) asked for: None, or dict(first, last, phase_edge, windows, axes, geospread, ranges) -- the array's
        seismometers first .. last inclusive (include/r3d_host.h r3dh_lapse_opts)."""
        rq = _ffi.LapseOpts()
        rc = self._lib.r3dh_lapse_request(self._h, C.byref(rq))
        if rc < 0:
            raise RuntimeError("lapse_request failed: " + self._lib.r3dh_last_error().decode())
        if rc == 0:
            return None
        return dict(first=int(rq.first), last=int(rq.last), phase_edge=tuple(rq.phase_edge), windows=tuple(rq.windows),
                    axes=tuple(rq.axes), geospread=rq.geospread, ranges=tuple(rq.ranges))

    @staticmethod
    def _lapse_opts(request):
        rq = _ffi.LapseOpts(size=C.sizeof(_ffi.LapseOpts), first=int(request["first"]), last=int(request["last"]),
                            geospread=float(request["geospread"]))
        for name in ("phase_edge", "windows", "axes", "ranges"):
            field = getattr(rq, name)
            if len(request[name]) != len(field):
                raise ValueError(f"lapse request: {name} needs {len(field)} numbers")
            for k, v in enumerate(request[name]):
                field[k] = float(v)
        return rq

    def lapse_plan(self, request=None):
        """(distances [S], bins [S, 2, 2], clipped [S, 2]) of the lapse array (`request`: a dict as lapse_request gives;
        None: the model's own): every receiver's epicentral distance as vis/seisplot/range_km.m takes it from
        seis_NNN.octv, and the begin, end bins of its two lapse windows (include/r3d.h r3d_window_bins)."""
        request = request if request is not None else self.lapse_request
        if request is None:
            raise RuntimeError("the model's arguments hold no --lapse-windows")
        rq = self._lapse_opts(request)
        S = int(rq.last) - int(rq.first) + 1
        if S < 1:
            raise ValueError("lapse request: first > last")
        dist, bins, clipped = np.zeros(S), np.zeros((S, 2, 2), dtype=np.uint32), np.zeros((S, 2), dtype=np.int32)
        if self._lib.r3dh_lapse_plan(self._h, C.byref(rq), dist.ctypes.data_as(_ffi._dp),
                                     bins.ctypes.data_as(C.POINTER(C.c_uint32)), clipped.ctypes.data_as(C.POINTER(C.c_int32))):
            raise RuntimeError("lapse_plan failed: " + self._lib.r3dh_last_error().decode())
        return dist, bins, clipped.astype(bool)

    def write_lapse(self, path, plan, window_energy, window_se, window_counts, batch_window_energy, request=None):
        """Write lapse.octv (include/r3d_host.h r3dh_write_lapse) to `path`: plan = lapse_plan(request); window_energy /
        window_se [S, 2], window_counts [S, 2, 2] and batch_window_energy [B, S, 2] the ARRAY's rows of what
        Engine.run_batched_windows returned for the plan's bins."""
        request = request if request is not None else self.lapse_request
        if request is None:
            raise RuntimeError("the model's arguments hold no --lapse-windows")
        rq = self._lapse_opts(request)
        S = int(rq.last) - int(rq.first) + 1
        dist = np.ascontiguousarray(plan[0], dtype=np.float64).reshape(S)
        bins = np.ascontiguousarray(plan[1], dtype=np.uint32).reshape(S, 2, 2)
        clipped = np.ascontiguousarray(plan[2], dtype=np.int32).reshape(S, 2)
        we = np.ascontiguousarray(window_energy, dtype=np.float64).reshape(S, 2)
        wse = np.ascontiguousarray(window_se, dtype=np.float64).reshape(S, 2)
        wc = np.ascontiguousarray(window_counts, dtype=np.uint64).reshape(S, 2, 2)
        bwe = np.ascontiguousarray(batch_window_energy, dtype=np.float64)
        B = bwe.shape[0]
        bwe = bwe.reshape(B, S, 2)
        res = _ffi.LapseResult(C.sizeof(_ffi.LapseResult), B, dist.ctypes.data, bins.ctypes.data, clipped.ctypes.data,
                               we.ctypes.data, wse.ctypes.data, wc.ctypes.data, bwe.ctypes.data)
        if self._lib.r3dh_write_lapse(self._h, C.byref(rq), C.byref(res), str(path).encode()):
            raise RuntimeError("write_lapse failed: " + self._lib.r3dh_last_error().decode())

    @property
    def ttimage_request(self):
        """What --ttimage[=GAMMA,NORM] and its companions (--ttimage-array, --ttimage-axes, --ttimage-fit,
        --ttimage-normcurve) asked for: None, or dict(first, last, gamma_log2, norm, axes, fit, curve) -- the array's
        seismometers first .. last inclusive, fit the 1-based (IBEGIN, IEND) or (0, 0), curve (C, Q) or NaNs
        (include/r3d_host.h r3dh_ttimage_opts)."""
        rq = _ffi.TTImageOpts()
        rc = self._lib.r3dh_ttimage_request(self._h, C.byref(rq))
        if rc < 0:
            raise RuntimeError("ttimage_request failed: " + self._lib.r3dh_last_error().decode())
        if rc == 0:
            return None
        return dict(first=int(rq.first), last=int(rq.last), gamma_log2=int(rq.gamma_log2), norm=rq.norm, axes=tuple(rq.axes),
                    fit=(int(rq.fit_begin), int(rq.fit_end)), curve=(rq.curve_c, rq.curve_q))

    @staticmethod
    def _ttimage_opts(request):
        fit, curve = request.get("fit", (0, 0)), request.get("curve", (math.nan, math.nan))
        return _ffi.TTImageOpts(size=C.sizeof(_ffi.TTImageOpts), first=int(request["first"]), last=int(request["last"]),
                                gamma_log2=int(request.get("gamma_log2", 1)), fit_begin=int(fit[0]), fit_end=int(fit[1]),
                                norm=float(request.get("norm", 0.3)),
                                axes=(C.c_double * 3)(*[float(v) for v in request.get("axes", (1, 1, 1))]),
                                curve_c=float(curve[0]), curve_q=float(curve[1]))

    def ttimage_plan(self, request=None):
        """(distances [A], azimuths [A]) of the image's array (`request`: a dict as ttimage_request gives, of which first
        and last are read; None: the model's own): every receiver's epicentral distance and azimuth as
        vis/seisplot/range_km.m and azimuth_deg.m take them from seis_NNN.octv."""
        request = request if request is not None else self.ttimage_request
        if request is None:
            raise RuntimeError("the model's arguments hold no --ttimage")
        rq = self._ttimage_opts(request)
        A = int(rq.last) - int(rq.first) + 1
        if A < 1:
            raise ValueError("ttimage request: first > last")
        dist, azi = np.zeros(A), np.zeros(A)
        if self._lib.r3dh_ttimage_plan(self._h, C.byref(rq), dist.ctypes.data_as(_ffi._dp), azi.ctypes.data_as(_ffi._dp)):
            raise RuntimeError("ttimage_plan failed: " + self._lib.r3dh_last_error().decode())
        return dist, azi

    def write_ttimage(self, path, plan, image, n_batches, request=None):
        """Write ttimage.octv (include/r3d_host.h r3dh_write_ttimage) to `path`: plan = ttimage_plan(request), image the
        dict Engine.run_batched_array_image returned for the request's array."""
        request = request if request is not None else self.ttimage_request
        if request is None:
            raise RuntimeError("the model's arguments hold no --ttimage")
        rq = self._ttimage_opts(request)
        keep = [np.ascontiguousarray(plan[0], dtype=np.float64), np.ascontiguousarray(plan[1], dtype=np.float64)]
        has_fit = "fit" in image
        for name, kind in (("image", np.float64), ("image_se", np.float64), ("lit", np.uint32), ("summed", np.float64),
                           ("summed_se", np.float64), ("peak", np.float64), ("peak_bin", np.uint32)):
            keep.append(np.ascontiguousarray(image[name], dtype=kind))
        res = _ffi.TTImageResult(C.sizeof(_ffi.TTImageResult), int(n_batches), int(has_fit), int(image.get("curve_made", 0)),
                                 *[a.ctypes.data for a in keep])
        if has_fit:
            for name in ("curve", "image_curve", "image_curve_se"):
                keep.append(np.ascontiguousarray(image[name], dtype=np.float64))
                setattr(res, name, keep[-1].ctypes.data)
            for k in range(2):
                res.fit[k], res.fit_se[k] = image["fit"][k], image["fit_se"][k]
        if self._lib.r3dh_write_ttimage(self._h, C.byref(rq), C.byref(res), str(path).encode()):
            raise RuntimeError("write_ttimage failed: " + self._lib.r3dh_last_error().decode())

    @property
    def envshape_request(self):
        """What --envelope-shape[=V,T0,O,E[,SMOOTH]] and its companions (--envelope-array, --envelope-axes) asked for: None,
        or dict(first, last, smooth, phase_edge, window, axes) -- the array's seismometers first .. last inclusive, window
        (O, E) in seconds behind the edge with E = NaN for "to the end of the trace" (include/r3d_host.h
        r3dh_envshape_opts)."""
        rq = _ffi.EnvShapeOpts()
        rc = self._lib.r3dh_envshape_request(self._h, C.byref(rq))
        if rc < 0:
            raise RuntimeError("envshape_request failed: " + self._lib.r3dh_last_error().decode())
        if rc == 0:
            return None
        return dict(first=int(rq.first), last=int(rq.last), smooth=int(rq.smooth), phase_edge=tuple(rq.phase_edge),
                    window=tuple(rq.window), axes=tuple(rq.axes))

    def slant_plan(self):
        """What --slant-stack and its companions asked for, planned for the model's array (include/r3d_host.h
        r3dh_slant_request, r3dh_slant_plan): None without the option, else a dict of first, last, smooth, amplitude, axes,
        distances [A] (km), r_ref, p0, dp (s/km), shift_bin, shift_frac [M, A], gain [A] and windows [W, 2] (bins)."""
        rq = _ffi.SlantOpts()
        rc = self._lib.r3dh_slant_request(self._h, C.byref(rq))
        if rc < 0:
            raise RuntimeError("slant_request failed: " + self._lib.r3dh_last_error().decode())
        if rc == 0:
            return None
        A, M, W = int(rq.last) - int(rq.first) + 1, int(rq.n_slowness), max(1, int(rq.n_windows))
        dist, grid, gain = np.zeros(A), np.zeros(3), np.zeros(A)
        k, f, win = np.zeros((M, A), dtype=np.int32), np.zeros((M, A)), np.zeros((W, 2), dtype=np.uint32)
        if self._lib.r3dh_slant_plan(self._h, C.byref(rq), dist.ctypes.data_as(_ffi._dp), grid.ctypes.data_as(_ffi._dp),
                                     k.ctypes.data_as(C.POINTER(C.c_int32)), f.ctypes.data_as(_ffi._dp),
                                     gain.ctypes.data_as(_ffi._dp), win.ctypes.data_as(C.POINTER(C.c_uint32))):
            raise RuntimeError("slant_plan failed: " + self._lib.r3dh_last_error().decode())
        return dict(first=int(rq.first), last=int(rq.last), smooth=int(rq.smooth), amplitude=int(rq.amplitude), axes=tuple(rq.axes),
                    distances=dist, r_ref=float(grid[0]), p0=float(grid[1]), dp=float(grid[2]), shift_bin=k, shift_frac=f, gain=gain,
                    windows=win)

    def contrast_plan(self):
        """What --array-contrast and its companions asked for, planned for the model's array (include/r3d_host.h
        r3dh_contrast_request, r3dh_contrast_plan): None without the option, else a dict of first, last, smooth, axes, test_args
        (--contrast-model-args), seed and num_phonons (the test run's), velocities [W, 2] (km/s), regions_km [R, 2], range_power,
        distances [A] (km), bins [A, W, 2], clipped [A, W], regions [R, 2] (indices into the array), gain [A] and r_ref."""
        rq = _ffi.ContrastOpts()
        rc = self._lib.r3dh_contrast_request(self._h, C.byref(rq))
        if rc < 0:
            raise RuntimeError("contrast_request failed: " + self._lib.r3dh_last_error().decode())
        if rc == 0:
            return None
        A, W, R = int(rq.last) - int(rq.first) + 1, int(rq.n_windows), int(rq.n_regions)
        dist, gain, ref = np.zeros(A), np.zeros(A), C.c_double()
        bins, cut, reg = np.zeros((A, W, 2), dtype=np.uint32), np.zeros((A, W), dtype=np.int32), np.zeros((R, 2), dtype=np.uint32)
        if self._lib.r3dh_contrast_plan(self._h, C.byref(rq), dist.ctypes.data_as(_ffi._dp), bins.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        cut.ctypes.data_as(C.POINTER(C.c_int32)), reg.ctypes.data_as(C.POINTER(C.c_uint32)),
                                        gain.ctypes.data_as(_ffi._dp), C.byref(ref)):
            raise RuntimeError("contrast_plan failed: " + self._lib.r3dh_last_error().decode())
        return dict(first=int(rq.first), last=int(rq.last), smooth=int(rq.smooth), axes=tuple(rq.axes),
                    test_args=[rq.test_args[k] for k in range(rq.n_test_args)], seed=int(rq.seed), num_phonons=int(rq.num_phonons),
                    velocities=np.array([tuple(rq.velocities[w]) for w in range(W)]).reshape(W, 2),
                    regions_km=np.array([tuple(rq.regions[r]) for r in range(R)]).reshape(R, 2), range_power=rq.range_power,
                    distances=dist, bins=bins, clipped=cut, regions=reg, gain=gain, r_ref=ref.value)

    @staticmethod
    def _envshape_opts(request):
        edge, window = request.get("phase_edge", (3.6, 0.0)), request.get("window", (0.0, math.nan))
        return _ffi.EnvShapeOpts(size=C.sizeof(_ffi.EnvShapeOpts), first=int(request["first"]), last=int(request["last"]),
                                 smooth=int(request.get("smooth", 8)), phase_edge=(C.c_double * 2)(*[float(v) for v in edge]),
                                 window=(C.c_double * 2)(*[float(v) for v in window]),
                                 axes=(C.c_double * 3)(*[float(v) for v in request.get("axes", (1, 1, 1))]))

    def envshape_plan(self, request=None):
        """(distances [A], bins [A, 2], clipped [A]) of the envelope array (`request`: a dict as envshape_request gives;
        None: the model's own): every receiver's epicentral distance as vis/seisplot/range_km.m takes it from
        seis_NNN.octv, and its window of bins b0, b1 (include/r3d.h r3d_window_bins; to the last bin where the window's E
        is NaN)."""
        request = request if request is not None else self.envshape_request
        if request is None:
            raise RuntimeError("the model's arguments hold no --envelope-shape")
        rq = self._envshape_opts(request)
        A = int(rq.last) - int(rq.first) + 1
        if A < 1:
            raise ValueError("envshape request: first > last")
        dist, bins, clipped = np.zeros(A), np.zeros((A, 2), dtype=np.uint32), np.zeros(A, dtype=np.int32)
        if self._lib.r3dh_envshape_plan(self._h, C.byref(rq), dist.ctypes.data_as(_ffi._dp),
                                        bins.ctypes.data_as(C.POINTER(C.c_uint32)), clipped.ctypes.data_as(C.POINTER(C.c_int32))):
            raise RuntimeError("envshape_plan failed: " + self._lib.r3dh_last_error().decode())
        return dist, bins, clipped

    def write_envshape(self, path, plan, shape, n_batches, request=None):
        """Write envshape.octv (include/r3d_host.h r3dh_write_envshape) to `path`: plan = envshape_plan(request), shape the
        dict Engine.run_batched_envelope_shape returned for the request's array."""
        request = request if request is not None else self.envshape_request
        if request is None:
            raise RuntimeError("the model's arguments hold no --envelope-shape")
        rq = self._envshape_opts(request)
        keep = [np.ascontiguousarray(plan[0], dtype=np.float64), np.ascontiguousarray(plan[1], dtype=np.uint32),
                np.ascontiguousarray(plan[2], dtype=np.int32)]
        for name, kind in (("shape", np.float64), ("shape_se", np.float64), ("envelope", np.float64), ("envelope_se", np.float64),
                           ("peak_bin", np.uint32), ("half_bin", np.uint32), ("lit", np.uint32)):
            keep.append(np.ascontiguousarray(shape[name], dtype=kind))
        res = _ffi.EnvShapeResult(C.sizeof(_ffi.EnvShapeResult), int(n_batches), *[a.ctypes.data for a in keep])
        if self._lib.r3dh_write_envshape(self._h, C.byref(rq), C.byref(res), str(path).encode()):
            raise RuntimeError("write_envshape failed: " + self._lib.r3dh_last_error().decode())

    @property
    def envbands_request(self):
        """What --envelope-bands=R,LEVEL[,V,T0,O,E[,SMOOTH]] and its companions (--bands-array, --bands-axes, --bands-seed) asked
        for: None, or dict(first, last, smooth, n_replicates, tail, level, seed, phase_edge, window, axes) -- tail is
        floor((0.5 (1 - level)) n_replicates), the window as envshape_request's (include/r3d_host.h r3dh_envbands_opts)."""
        rq = _ffi.EnvBandsOpts()
        rc = self._lib.r3dh_envbands_request(self._h, C.byref(rq))
        if rc < 0:
            raise RuntimeError("envbands_request failed: " + self._lib.r3dh_last_error().decode())
        if rc == 0:
            return None
        return dict(first=int(rq.first), last=int(rq.last), smooth=int(rq.smooth), n_replicates=int(rq.n_replicates),
                    tail=int(rq.tail), level=float(rq.level), seed=int(rq.seed), phase_edge=tuple(rq.phase_edge),
                    window=tuple(rq.window), axes=tuple(rq.axes))

    @staticmethod
    def _envbands_opts(request):
        edge, window = request.get("phase_edge", (3.6, 0.0)), request.get("window", (0.0, math.nan))
        R, level = int(request.get("n_replicates", 1000)), float(request.get("level", 0.9))
        return _ffi.EnvBandsOpts(size=C.sizeof(_ffi.EnvBandsOpts), first=int(request["first"]), last=int(request["last"]),
                                 smooth=int(request.get("smooth", 8)), n_replicates=R, tail=int(request.get("tail", bands_tail(R, level))),
                                 seed=int(request.get("seed", 0xB007)), level=level,
                                 phase_edge=(C.c_double * 2)(*[float(v) for v in edge]),
                                 window=(C.c_double * 2)(*[float(v) for v in window]),
                                 axes=(C.c_double * 3)(*[float(v) for v in request.get("axes", (1, 1, 1))]))

    def envbands_plan(self, request=None):
        """(distances [A], bins [A, 2], clipped [A]) of the bands' array (`request`: a dict as envbands_request gives; None: the
        model's own): envshape_plan's rule for the request's array and window (include/r3d_host.h r3dh_envbands_plan)."""
        request = request if request is not None else self.envbands_request
        if request is None:
            raise RuntimeError("the model's arguments hold no --envelope-bands")
        rq = self._envbands_opts(request)
        A = int(rq.last) - int(rq.first) + 1
        if A < 1:
            raise ValueError("envbands request: first > last")
        dist, bins, clipped = np.zeros(A), np.zeros((A, 2), dtype=np.uint32), np.zeros(A, dtype=np.int32)
        if self._lib.r3dh_envbands_plan(self._h, C.byref(rq), dist.ctypes.data_as(_ffi._dp),
                                        bins.ctypes.data_as(C.POINTER(C.c_uint32)), clipped.ctypes.data_as(C.POINTER(C.c_int32))):
            raise RuntimeError("envbands_plan failed: " + self._lib.r3dh_last_error().decode())
        return dist, bins, clipped

    def write_envbands(self, path, plan, bands, n_batches, request=None):
        """Write envbands.octv (include/r3d_host.h r3dh_write_envbands) to `path`: plan = envbands_plan(request), bands the dict
        Engine.run_batched_envelope_bands returned for the request's array."""
        request = request if request is not None else self.envbands_request
        if request is None:
            raise RuntimeError("the model's arguments hold no --envelope-bands")
        rq = self._envbands_opts(request)
        keep = [np.ascontiguousarray(plan[0], dtype=np.float64), np.ascontiguousarray(plan[1], dtype=np.uint32),
                np.ascontiguousarray(plan[2], dtype=np.int32)]
        for name in ("envelope", "envelope_lo", "envelope_hi", "shape", "shape_lo", "shape_hi"):
            keep.append(np.ascontiguousarray(bands[name], dtype=np.float64))
        keep.append(np.ascontiguousarray(bands["defined"], dtype=np.uint32))
        res = _ffi.EnvBandsResult(C.sizeof(_ffi.EnvBandsResult), int(n_batches), *[a.ctypes.data for a in keep])
        if self._lib.r3dh_write_envbands(self._h, C.byref(rq), C.byref(res), str(path).encode()):
            raise RuntimeError("write_envbands failed: " + self._lib.r3dh_last_error().decode())

    @property
    def envfit_request(self):
        """What --envelope-fit=FILE[,V,T0,O,E[,SMOOTH[,OBSSMOOTH[,MAXLAG_SECONDS]]]] and its companions (--envelope-fit-array,
        --envelope-fit-axes, --envelope-fit-energy) asked for: None, or dict(file, first, last, smooth_syn, smooth_obs,
        amplitude, energy_file, phase_edge, window, axes, max_lag_seconds) (include/r3d_host.h r3dh_envfit_opts)."""
        rq = _ffi.EnvFitOpts()
        rc = self._lib.r3dh_envfit_request(self._h, C.byref(rq))
        if rc < 0:
            raise RuntimeError("envfit_request failed: " + self._lib.r3dh_last_error().decode())
        if rc == 0:
            return None
        return dict(file=rq.file.decode(), first=int(rq.first), last=int(rq.last), smooth_syn=int(rq.smooth_syn),
                    smooth_obs=int(rq.smooth_obs), amplitude=int(rq.amplitude), energy_file=int(rq.energy_file),
                    phase_edge=tuple(rq.phase_edge), window=tuple(rq.window), axes=tuple(rq.axes),
                    max_lag_seconds=float(rq.max_lag_seconds))

    @staticmethod
    def _envfit_opts(request):
        edge, window = request.get("phase_edge", (3.6, 0.0)), request.get("window", (0.0, math.nan))
        return _ffi.EnvFitOpts(size=C.sizeof(_ffi.EnvFitOpts), first=int(request["first"]), last=int(request["last"]),
                               smooth_syn=int(request.get("smooth_syn", 8)), smooth_obs=int(request.get("smooth_obs", 0)),
                               amplitude=int(request.get("amplitude", 1)), energy_file=int(request.get("energy_file", 0)),
                               phase_edge=(C.c_double * 2)(*[float(v) for v in edge]),
                               window=(C.c_double * 2)(*[float(v) for v in window]),
                               axes=(C.c_double * 3)(*[float(v) for v in request.get("axes", (1, 1, 1))]),
                               max_lag_seconds=float(request.get("max_lag_seconds", 0.0)), file=str(request["file"]).encode())

    def envfit_plan(self, request=None):
        """(distances [A], bins [A, 2], clipped [A], observed [A, n_bins], max_lag) of the fit's array (`request`: a dict as
        envfit_request gives; None: the model's own): the envelope shape's window rule (envshape_plan), the observed
        envelopes of the request's file resampled onto the run's bins (observed_to_bins; their roots where the file holds
        energies and amplitudes are compared) and the largest lag in bins."""
        request = request if request is not None else self.envfit_request
        if request is None:
            raise RuntimeError("the model's arguments hold no --envelope-fit")
        rq = self._envfit_opts(request)
        A = int(rq.last) - int(rq.first) + 1
        if A < 1:
            raise ValueError("envfit request: first > last")
        dist, bins, clipped = np.zeros(A), np.zeros((A, 2), dtype=np.uint32), np.zeros(A, dtype=np.int32)
        observed, max_lag = np.zeros((A, self.n_bins)), C.c_uint32(0)
        if self._lib.r3dh_envfit_plan(self._h, C.byref(rq), dist.ctypes.data_as(_ffi._dp), bins.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      clipped.ctypes.data_as(C.POINTER(C.c_int32)), observed.ctypes.data_as(_ffi._dp),
                                      C.byref(max_lag)):
            raise RuntimeError("envfit_plan failed: " + self._lib.r3dh_last_error().decode())
        return dist, bins, clipped, observed, int(max_lag.value)

    def write_envfit(self, path, plan, fit, n_batches, request=None):
        """Write envfit.octv (include/r3d_host.h r3dh_write_envfit) to `path`: plan = envfit_plan(request), fit the dict
        Engine.run_batched_envelope_misfit returned for the request's array and the plan's lag."""
        request = request if request is not None else self.envfit_request
        if request is None:
            raise RuntimeError("the model's arguments hold no --envelope-fit")
        rq = self._envfit_opts(request)
        keep = [np.ascontiguousarray(plan[0], dtype=np.float64), np.ascontiguousarray(plan[1], dtype=np.uint32),
                np.ascontiguousarray(plan[2], dtype=np.int32), np.ascontiguousarray(plan[3], dtype=np.float64)]
        for name in ("misfit", "misfit_se", "xcorr", "xcorr_se", "envelope"):
            keep.append(np.ascontiguousarray(fit[name], dtype=np.float64))
        keep.append(np.ascontiguousarray(fit["lit"], dtype=np.uint32))
        if keep[6].shape[-1] != 2 * int(plan[4]) + 1:
            raise ValueError("the fit's xcorr has not the plan's 2 max_lag + 1 lags")
        res = _ffi.EnvFitResult(C.sizeof(_ffi.EnvFitResult), int(n_batches), int(plan[4]), 0, *[a.ctypes.data for a in keep])
        if self._lib.r3dh_write_envfit(self._h, C.byref(rq), C.byref(res), str(path).encode()):
            raise RuntimeError("write_envfit failed: " + self._lib.r3dh_last_error().decode())

    def new_result(self):
        return Result(self.n_seismometers, self.n_bins)


def batch_moments(batch_energy, batch_counts, batch_scalars=None, energy=None, counts=None, scalars=None, stream=None):
    """r3d_batch_moments on torch tensors of one device: batch_energy [B, ...] float64 and batch_counts [B, ...] of
    a 64-bit integer type are B batch blocks (batch_scalars [B, k] likewise, optional).  Returns
    (energy, counts, scalars, energy_se, counts_se): the blocks' sums ADDED into `energy` / `counts` / `scalars`
    (made and zeroed here when None; scalars is None without batch_scalars) and the standard errors of those sums
    (include/r3d.h has the estimator).  Asynchronous on `stream` (a raw hipStream_t; None: torch's current one)."""
    import torch
    lib = _ffi.hip_lib()
    B = int(batch_energy.shape[0])
    for t, what in ((batch_energy, torch.float64), (batch_counts, None), (batch_scalars, None)):
        if t is None:
            continue
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != 8 or t.shape[0] != B or t.device != batch_energy.device:
            raise ValueError("batch blocks must be contiguous 8-byte tensors [B, ...] on one GPU")
        if (what is not None and t.dtype != what) or (what is None and t.dtype.is_floating_point):
            raise ValueError("batch_energy must be float64, batch_counts / batch_scalars 64-bit integers")
    dev = batch_energy.device
    if energy is None:
        energy = torch.zeros(batch_energy.shape[1:], dtype=torch.float64, device=dev)
    if counts is None:
        counts = torch.zeros(batch_counts.shape[1:], dtype=batch_counts.dtype, device=dev)
    if scalars is None and batch_scalars is not None:
        scalars = torch.zeros(batch_scalars.shape[1:], dtype=batch_scalars.dtype, device=dev)
    ne, nc = batch_energy[0].numel(), batch_counts[0].numel()
    for t, n in ((energy, ne), (counts, nc)):
        if t.device != dev or not t.is_contiguous() or t.numel() != n or t.element_size() != 8:
            raise ValueError("totals must be contiguous 8-byte tensors of a block's size on the blocks' GPU")
    energy_se = torch.empty(batch_energy.shape[1:], dtype=torch.float64, device=dev)
    counts_se = torch.empty(batch_counts.shape[1:], dtype=torch.float64, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.r3d_batch_moments(dev.index or 0, B, batch_energy.data_ptr(), ne, batch_counts.data_ptr(), nc,
                               batch_scalars.data_ptr() if batch_scalars is not None else None,
                               batch_scalars[0].numel() if batch_scalars is not None else 0,
                               energy.data_ptr(), counts.data_ptr(), scalars.data_ptr() if scalars is not None else None,
                               energy_se.data_ptr(), counts_se.data_ptr(), stream)
    if rc:
        raise RuntimeError("r3d_batch_moments failed: " + lib.r3d_last_error().decode())
    return energy, counts, scalars, energy_se, counts_se


def window_spec(n_seismometers, n_bins, n_windows, bins_ptr, weights):
    """An r3d_window_spec (include/r3d.h): bins_ptr the address of the uint32 [n_seis][n_windows][2] begin, end pairs --
    on the device for window_sums, on the host for Engine.run_batched_windows."""
    w = [float(v) for v in weights]
    if len(w) != _ffi.R3D_N_ENERGY:
        raise ValueError("five component weights (X, Y, Z, P, S) are needed")
    return _ffi.WindowSpec(C.sizeof(_ffi.WindowSpec), int(n_seismometers), int(n_bins), int(n_windows), bins_ptr,
                           (C.c_double * _ffi.R3D_N_ENERGY)(*w))


def window_bins(dt, n_bins, r, v, t0, o, e):
    """r3d_window_bins: (begin, end, clipped) -- the 0-based half-open bins of the window that runs from o to e seconds
    behind the phase edge (v, t0) at epicentral distance r, bins of dt seconds (vis/seisplot/lapsetimecurve.m's rule;
    include/r3d.h).  clipped: the rule's bins did not fit [0, n_bins) and were cut.  Needs no GPU."""
    lib = _ffi.hip_lib()
    out, clipped = (C.c_uint32 * 2)(), C.c_int(0)
    if lib.r3d_window_bins(float(dt), int(n_bins), float(r), float(v), float(t0), float(o), float(e), out, C.byref(clipped)):
        raise RuntimeError("r3d_window_bins failed: " + lib.r3d_last_error().decode())
    return int(out[0]), int(out[1]), bool(clipped.value)


def window_log_ratio(a, b):
    """r3d_window_log_ratio: (theta, se) -- log10(sum a / sum b) of N batch values each and its jackknife standard
    error; both NaN where a full or a leave-one-out sum is not positive (include/r3d.h).  Needs no GPU."""
    lib = _ffi.hip_lib()
    a, b = np.ascontiguousarray(a, dtype=np.float64).reshape(-1), np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    if a.size != b.size:
        raise ValueError("a and b must hold one value per batch each")
    theta, se = C.c_double(), C.c_double()
    if lib.r3d_window_log_ratio(a.size, a.ctypes.data_as(_ffi._dp), b.ctypes.data_as(_ffi._dp), 1, C.byref(theta),
                                C.byref(se)):
        raise RuntimeError("r3d_window_log_ratio failed: " + lib.r3d_last_error().decode())
    return theta.value, se.value


def window_sums(batch_energy, bins, weights, batch_counts=None, window_energy=None, window_counts=None, count_bad=False,
                stream=None):
    """r3d_window_sums on torch tensors of one device: batch_energy [B, S, n_bins, 5] float64 (and batch_counts
    [B, S, n_bins, 2] of a 64-bit integer type, optional) are B batch blocks, bins [S, W, 2] int32 the begin, end pairs
    of W windows per seismometer, weights the five component weights.  Returns (window_energy [B, S, W], window_counts
    [B, S, W, 2] or None, bad): every block's weighted sum over every window, WRITTEN (into the tensors given, or new
    ones); bad is a one-element tensor with the number of pairs that are not begin <= end <= n_bins (count_bad), else
    None.  The result is one more batch-major block: batch_moments turns it into totals and standard errors.
    Asynchronous on `stream` (a raw hipStream_t; None: torch's current one)."""
    import torch
    lib = _ffi.hip_lib()
    if batch_energy.dim() != 4 or batch_energy.shape[3] != _ffi.R3D_N_ENERGY or batch_energy.dtype != torch.float64:
        raise ValueError("batch_energy must be float64 [B, S, n_bins, 5]")
    B, S, n_bins = (int(v) for v in batch_energy.shape[:3])
    dev = batch_energy.device
    if bins.dim() != 3 or bins.shape[0] != S or bins.shape[2] != 2 or bins.element_size() != 4 or bins.dtype.is_floating_point:
        raise ValueError("bins must be a 32-bit integer tensor [S, W, 2]")
    W = int(bins.shape[1])
    tensors = [batch_energy, bins]
    if batch_counts is not None:
        if tuple(batch_counts.shape) != (B, S, n_bins, _ffi.R3D_N_COUNT) or batch_counts.element_size() != 8 \
                or batch_counts.dtype.is_floating_point:
            raise ValueError("batch_counts must be a 64-bit integer tensor [B, S, n_bins, 2]")
        tensors.append(batch_counts)
        if window_counts is None:
            window_counts = torch.empty((B, S, W, _ffi.R3D_N_COUNT), dtype=batch_counts.dtype, device=dev)
        tensors.append(window_counts)
    if window_energy is None:
        window_energy = torch.empty((B, S, W), dtype=torch.float64, device=dev)
    tensors.append(window_energy)
    for t in tensors:
        if not t.is_cuda or not t.is_contiguous() or t.device != dev:
            raise ValueError("blocks, bins and outputs must be contiguous tensors on one GPU")
    if window_energy.numel() != B * S * W or window_energy.dtype != torch.float64:
        raise ValueError("window_energy must be float64 [B, S, W]")
    if window_counts is not None and (window_counts.numel() != 2 * B * S * W or window_counts.element_size() != 8):
        raise ValueError("window_counts must be a 64-bit integer tensor [B, S, W, 2]")
    bad = torch.zeros(1, dtype=torch.int64, device=dev) if count_bad else None
    spec = window_spec(S, n_bins, W, bins.data_ptr(), weights)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.r3d_window_sums(dev.index or 0, B, batch_energy.data_ptr(),
                             batch_counts.data_ptr() if batch_counts is not None else None, C.byref(spec),
                             window_energy.data_ptr(), window_counts.data_ptr() if window_counts is not None else None,
                             bad.data_ptr() if bad is not None else None, stream)
    if rc:
        raise RuntimeError("r3d_window_sums failed: " + lib.r3d_last_error().decode())
    return window_energy, window_counts, bad


def array_image_spec(n_seismometers, n_bins, first, last, weights, gamma_log2=1, rho=0.3, curve_ptr=None, window_length=0.0,
                     fit=(0, 0), ranges=(0.0, 0.0), curve=(math.nan, math.nan)):
    """An r3d_array_image_spec (include/r3d.h): LEGACY mode with the norm ratio `rho`, or -- with curve_ptr, the device
    address of the array's [A] curve values -- CURVE mode with window_length = n_bins * dt.  fit (1-based IBEGIN, IEND),
    ranges (the distances of receivers first and last) and curve (c, q given outright) are read by
    Engine.run_batched_array_image only."""
    w = [float(v) for v in weights]
    if len(w) != _ffi.R3D_N_ENERGY:
        raise ValueError("five component weights (X, Y, Z, P, S) are needed")
    return _ffi.ArrayImageSpec(size=C.sizeof(_ffi.ArrayImageSpec), n_seismometers=int(n_seismometers), n_bins=int(n_bins),
                               first=int(first), last=int(last), gamma_log2=int(gamma_log2),
                               mode=_ffi.R3D_ARRAY_CURVE if curve_ptr else _ffi.R3D_ARRAY_LEGACY, fit_begin=int(fit[0]),
                               fit_end=int(fit[1]), weight=(C.c_double * _ffi.R3D_N_ENERGY)(*w), rho=float(rho),
                               d_curve=curve_ptr, window_length=float(window_length),
                               range=(C.c_double * 2)(float(ranges[0]), float(ranges[1])), curve_c=float(curve[0]),
                               curve_q=float(curve[1]))


def array_image(batch_energy, first, last, weights, gamma_log2=1, rho=0.3, curve=None, window_length=0.0, with_se=None,
                image=None, image_se=None, stream=None):
    """r3d_array_image on torch tensors of one device: batch_energy [B, S, n_bins, 5] float64 are B batch blocks, the array
    the receivers first .. last (A of them), weights the five component weights (>= 0).  LEGACY mode with the norm ratio
    rho, or CURVE mode with `curve` (float64 [A] on the device) and window_length = n_bins * dt.  Returns a dict of
    tensors, all WRITTEN: image [A, n_bins], image_se [A, n_bins] (with_se; default: B >= 2), row_sum [B, A], peak [A],
    peak_bin [A] and lit [A] (int32), bad [1] (int64: the bad curve values).  include/r3d.h has the arithmetic.
    Asynchronous on `stream` (a raw hipStream_t; None: torch's current one)."""
    import torch
    lib = _ffi.hip_lib()
    if batch_energy.dim() != 4 or batch_energy.shape[3] != _ffi.R3D_N_ENERGY or batch_energy.dtype != torch.float64:
        raise ValueError("batch_energy must be float64 [B, S, n_bins, 5]")
    if not batch_energy.is_cuda or not batch_energy.is_contiguous():
        raise ValueError("the blocks must be a contiguous tensor on a GPU")
    B, S, n_bins = (int(v) for v in batch_energy.shape[:3])
    dev = batch_energy.device
    A = int(last) - int(first) + 1
    if A < 1 or last >= S:
        raise ValueError("the array first .. last must lie within the blocks' seismometers")
    if curve is not None and (curve.dtype != torch.float64 or curve.numel() != A or curve.device != dev or not curve.is_contiguous()):
        raise ValueError("curve must be float64 [A] on the blocks' GPU")
    with_se = B >= 2 if with_se is None else with_se
    if image is None:
        image = torch.empty((A, n_bins), dtype=torch.float64, device=dev)
    if image_se is None and with_se:
        image_se = torch.empty((A, n_bins), dtype=torch.float64, device=dev)
    for t in (image, image_se):
        if t is not None and (t.numel() != A * n_bins or t.dtype != torch.float64 or t.device != dev or not t.is_contiguous()):
            raise ValueError("image and image_se must be contiguous float64 [A, n_bins] on the blocks' GPU")
    out = dict(image=image, image_se=image_se, row_sum=torch.empty((B, A), dtype=torch.float64, device=dev),
               peak=torch.empty(A, dtype=torch.float64, device=dev), peak_bin=torch.empty(A, dtype=torch.int32, device=dev),
               lit=torch.empty(A, dtype=torch.int32, device=dev), bad=torch.zeros(1, dtype=torch.int64, device=dev))
    spec = array_image_spec(S, n_bins, first, last, weights, gamma_log2, rho, curve.data_ptr() if curve is not None else None,
                            window_length)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.r3d_array_image(dev.index or 0, B, batch_energy.data_ptr(), C.byref(spec), image.data_ptr(),
                             image_se.data_ptr() if image_se is not None else None, out["row_sum"].data_ptr(),
                             out["peak"].data_ptr(), out["peak_bin"].data_ptr(), out["lit"].data_ptr(), out["bad"].data_ptr(),
                             stream)
    if rc:
        raise RuntimeError("r3d_array_image failed: " + lib.r3d_last_error().decode())
    return out


def array_powerlaw(y, r_first, r_last, ibegin, iend):
    """r3d_array_powerlaw / r3d_array_powerlaw_jackknife (include/r3d.h; no GPU needed): the power law Y = c X^q over the
    1-based inclusive points ibegin .. iend of an array whose X runs evenly from r_first to r_last.  y [A]: returns
    (ln c, q).  y [B, A] batch values: returns (ln c, q, se(ln c), se(q), total [A]) of the batches' totals."""
    lib = _ffi.hip_lib()
    y = np.ascontiguousarray(y, dtype=np.float64)
    fit, se = (C.c_double * 2)(), (C.c_double * 2)()
    if y.ndim == 1:
        if lib.r3d_array_powerlaw(y.size, float(r_first), float(r_last), y.ctypes.data_as(_ffi._dp), 1, int(ibegin), int(iend), fit):
            raise RuntimeError("r3d_array_powerlaw failed: " + lib.r3d_last_error().decode())
        return fit[0], fit[1]
    B, A = y.shape
    total = np.zeros(A)
    if lib.r3d_array_powerlaw_jackknife(A, float(r_first), float(r_last), B, y.ctypes.data_as(_ffi._dp), A, int(ibegin),
                                        int(iend), fit, se, total.ctypes.data_as(_ffi._dp)):
        raise RuntimeError("r3d_array_powerlaw_jackknife failed: " + lib.r3d_last_error().decode())
    return fit[0], fit[1], se[0], se[1], total


def envelope_spec(n_seismometers, n_bins, first, last, weights, smooth, bins_ptr):
    """An r3d_envelope_spec (include/r3d.h): bins_ptr the address of the uint32 [A][2] b0, b1 pairs of the array's receivers
    first .. last -- on the device for envelope_shape, on the host for Engine.run_batched_envelope_shape."""
    w = [float(v) for v in weights]
    if len(w) != _ffi.R3D_N_ENERGY:
        raise ValueError("five component weights (X, Y, Z, P, S) are needed")
    return _ffi.EnvelopeSpec(size=C.sizeof(_ffi.EnvelopeSpec), n_seismometers=int(n_seismometers), n_bins=int(n_bins),
                             first=int(first), last=int(last), smooth=int(smooth), d_bins=bins_ptr,
                             weight=(C.c_double * _ffi.R3D_N_ENERGY)(*w))


def envelope_shape(batch_energy, bins, first, last, weights, smooth=8, with_se=None, with_envelope=True, stream=None):
    """r3d_envelope_shape on torch tensors of one device: batch_energy [B, S, n_bins, 5] float64 are B batch blocks, the array
    the receivers first .. last (A of them), bins [A, 2] int32 each receiver's window of bins b0, b1, weights the five
    component weights (>= 0), smooth the three-point passes.  Returns a dict of tensors, all WRITTEN: shape [A, 6] (E, P, peak
    time, half time, centroid, width; times in bins from the window's first bin), shape_se [A, 6] (with_se; default: B >=
    2), envelope and envelope_se [A, n_bins] (with_envelope), peak_bin, half_bin and lit [A] (int32; -1: dead / undecayed),
    bad [1] (int64: the windows that are not b0 <= b1 <= n_bins).  include/r3d.h has the arithmetic.  Asynchronous on
    `stream` (a raw hipStream_t; None: torch's current one)."""
    import torch
    lib = _ffi.hip_lib()
    if batch_energy.dim() != 4 or batch_energy.shape[3] != _ffi.R3D_N_ENERGY or batch_energy.dtype != torch.float64:
        raise ValueError("batch_energy must be float64 [B, S, n_bins, 5]")
    if not batch_energy.is_cuda or not batch_energy.is_contiguous():
        raise ValueError("the blocks must be a contiguous tensor on a GPU")
    B, S, n_bins = (int(v) for v in batch_energy.shape[:3])
    dev = batch_energy.device
    A = int(last) - int(first) + 1
    if A < 1 or last >= S:
        raise ValueError("the array first .. last must lie within the blocks' seismometers")
    if tuple(bins.shape) != (A, 2) or bins.element_size() != 4 or bins.dtype.is_floating_point or bins.device != dev \
            or not bins.is_contiguous():
        raise ValueError("bins must be a contiguous 32-bit integer tensor [A, 2] on the blocks' GPU")
    with_se = B >= 2 if with_se is None else with_se

    def f64(*shape):
        return torch.empty(shape, dtype=torch.float64, device=dev)

    def i32():
        return torch.empty(A, dtype=torch.int32, device=dev)
    out = dict(shape=f64(A, _ffi.R3D_ENVELOPE_N_SHAPE), shape_se=f64(A, _ffi.R3D_ENVELOPE_N_SHAPE) if with_se else None,
               envelope=f64(A, n_bins) if with_envelope else None, envelope_se=f64(A, n_bins) if with_envelope and with_se else None,
               peak_bin=i32(), half_bin=i32(), lit=i32(), bad=torch.zeros(1, dtype=torch.int64, device=dev))
    spec = envelope_spec(S, n_bins, first, last, weights, smooth, bins.data_ptr())
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    ptr = {k: (v.data_ptr() if v is not None else None) for k, v in out.items()}
    rc = lib.r3d_envelope_shape(dev.index or 0, B, batch_energy.data_ptr(), C.byref(spec), ptr["shape"], ptr["shape_se"],
                                ptr["envelope"], ptr["envelope_se"], ptr["peak_bin"], ptr["half_bin"], ptr["lit"], ptr["bad"],
                                stream)
    if rc:
        raise RuntimeError("r3d_envelope_shape failed: " + lib.r3d_last_error().decode())
    return out


def bands_spec(n_seismometers, n_bins, first, last, weights, smooth, n_replicates, tail, seed, bins_ptr):
    """An r3d_bands_spec (include/r3d.h): an envelope_spec's fields with the replicates R, the tail T (2 T < R) and the seed of
    the resampling counts."""
    w = [float(v) for v in weights]
    if len(w) != _ffi.R3D_N_ENERGY:
        raise ValueError("five component weights (X, Y, Z, P, S) are needed")
    return _ffi.BandsSpec(size=C.sizeof(_ffi.BandsSpec), n_seismometers=int(n_seismometers), n_bins=int(n_bins),
                          first=int(first), last=int(last), smooth=int(smooth), n_replicates=int(n_replicates), tail=int(tail),
                          d_bins=bins_ptr, seed=int(seed) & (2 ** 64 - 1), weight=(C.c_double * _ffi.R3D_N_ENERGY)(*w))


def bands_tail(n_replicates, level):
    """The tail T that ./main --envelope-bands=R,LEVEL takes: floor((0.5 (1 - LEVEL)) R); the achieved level is 1 - 2 T / R."""
    return int(math.floor((0.5 * (1.0 - float(level))) * float(n_replicates)))


def bootstrap_counts(seed, n_batches, n_replicates):
    """r3d_bootstrap_counts (host): the resampling counts [R, B] uint8 of the seed, every row summing to B."""
    lib = _ffi.hip_lib()
    counts = np.zeros((max(int(n_replicates), 0), max(int(n_batches), 0)), dtype=np.uint8)
    if lib.r3d_bootstrap_counts(int(seed) & (2 ** 64 - 1), int(n_batches), int(n_replicates), counts.ctypes.data):
        raise RuntimeError("r3d_bootstrap_counts failed: " + lib.r3d_last_error().decode())
    return counts


def envelope_bands(batch_energy, bins, first, last, weights, smooth=8, n_replicates=1000, tail=50, seed=0xB007, with_envelope=True,
                   stream=None):
    """r3d_envelope_bands on torch tensors of one device: batch_energy [B, S, n_bins, 5] float64 are B >= 2 batch blocks, the
    array the receivers first .. last (A of them), bins [A, 2] int32 each receiver's window of bins b0, b1, weights the five
    component weights (>= 0), smooth the three-point passes; the batches are resampled n_replicates times by the counts of
    `seed`, and tail values are left outside either band (2 tail < n_replicates).  Returns a dict of tensors, all WRITTEN:
    envelope, envelope_lo, envelope_hi [A, n_bins] (with_envelope), shape, shape_lo, shape_hi [A, 6], defined [A, 6] (int32: the
    replicates whose number is not NaN), bad [1] (int64).  include/r3d.h has the arithmetic.  Asynchronous on `stream` (a raw
    hipStream_t; None: torch's current one)."""
    import torch
    lib = _ffi.hip_lib()
    if batch_energy.dim() != 4 or batch_energy.shape[3] != _ffi.R3D_N_ENERGY or batch_energy.dtype != torch.float64:
        raise ValueError("batch_energy must be float64 [B, S, n_bins, 5]")
    if not batch_energy.is_cuda or not batch_energy.is_contiguous():
        raise ValueError("the blocks must be a contiguous tensor on a GPU")
    B, S, n_bins = (int(v) for v in batch_energy.shape[:3])
    dev = batch_energy.device
    A = int(last) - int(first) + 1
    if A < 1 or last >= S:
        raise ValueError("the array first .. last must lie within the blocks' seismometers")
    if tuple(bins.shape) != (A, 2) or bins.element_size() != 4 or bins.dtype.is_floating_point or bins.device != dev \
            or not bins.is_contiguous():
        raise ValueError("bins must be a contiguous 32-bit integer tensor [A, 2] on the blocks' GPU")

    def f64(*shape):
        return torch.empty(shape, dtype=torch.float64, device=dev)
    names = ("envelope", "envelope_lo", "envelope_hi", "shape", "shape_lo", "shape_hi", "defined", "bad")
    out = {k: (f64(A, n_bins) if with_envelope else None) for k in names[:3]}
    out.update({k: f64(A, _ffi.R3D_ENVELOPE_N_SHAPE) for k in names[3:6]})
    out["defined"] = torch.empty((A, _ffi.R3D_ENVELOPE_N_SHAPE), dtype=torch.int32, device=dev)
    out["bad"] = torch.zeros(1, dtype=torch.int64, device=dev)
    spec = bands_spec(S, n_bins, first, last, weights, smooth, n_replicates, tail, seed, bins.data_ptr())
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.r3d_envelope_bands(dev.index or 0, B, batch_energy.data_ptr(), C.byref(spec),
                                *[out[k].data_ptr() if out[k] is not None else None for k in names], stream)
    if rc:
        raise RuntimeError("r3d_envelope_bands failed: " + lib.r3d_last_error().decode())
    return out


def observed_to_bins(samples, t0, t1, t_begin, t_end, n_bins):
    """r3dh_observed_to_bins (include/r3d_host.h): the observed envelope `samples` (sample i at t0 + i (t1 - t0) / (n - 1))
    resampled by linear interpolation at linspace(t_begin, t_end, n_bins); +0.0 outside the observed span."""
    lib = _ffi.host_lib()
    v = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
    out = np.full(max(int(n_bins), 0), -7.0)
    if lib.r3dh_observed_to_bins(v.ctypes.data_as(_ffi._dp), v.size, 1, float(t0), float(t1), float(t_begin), float(t_end),
                                 int(n_bins), out.ctypes.data_as(_ffi._dp)):
        raise RuntimeError(lib.r3dh_last_error().decode())
    return out


def read_octave(path, name):
    """r3dh_read_octave (include/r3d_host.h): the variable `name` of a GNU/Octave text file of `scalar` and `matrix` blocks,
    as a float64 array [rows, cols]."""
    lib = _ffi.host_lib()
    rows, cols = C.c_uint32(0), C.c_uint32(0)
    if lib.r3dh_read_octave(str(path).encode(), name.encode(), C.byref(rows), C.byref(cols), None, 0):
        raise RuntimeError(lib.r3dh_last_error().decode())
    out = np.zeros((rows.value, cols.value))
    if lib.r3dh_read_octave(str(path).encode(), name.encode(), C.byref(rows), C.byref(cols), out.ctypes.data_as(_ffi._dp), out.size):
        raise RuntimeError(lib.r3dh_last_error().decode())
    return out


def misfit_spec(n_seismometers, n_bins, first, last, weights, bins_ptr, observed_ptr, smooth_syn=8, smooth_obs=0, max_lag=0,
                amplitude=1):
    """An r3d_misfit_spec (include/r3d.h): bins_ptr the address of the uint32 [A][2] b0, b1 pairs of the array's receivers
    first .. last, observed_ptr that of the float64 [A][n_bins] observed amplitudes on the run's bins -- both on the device
    for envelope_misfit, on the host for Engine.run_batched_envelope_misfit."""
    w = [float(v) for v in weights]
    if len(w) != _ffi.R3D_N_ENERGY:
        raise ValueError("five component weights (X, Y, Z, P, S) are needed")
    return _ffi.MisfitSpec(size=C.sizeof(_ffi.MisfitSpec), n_seismometers=int(n_seismometers), n_bins=int(n_bins),
                           first=int(first), last=int(last), smooth_syn=int(smooth_syn), smooth_obs=int(smooth_obs),
                           max_lag=int(max_lag), amplitude=int(amplitude), d_bins=bins_ptr, d_observed=observed_ptr,
                           weight=(C.c_double * _ffi.R3D_N_ENERGY)(*w))


def envelope_misfit(batch_energy, bins, observed, first, last, weights, smooth_syn=8, smooth_obs=0, max_lag=0, amplitude=1,
                    with_se=None, with_xcorr=True, with_envelope=True, stream=None):
    """r3d_envelope_misfit on torch tensors of one device: batch_energy [B, S, n_bins, 5] float64 are B batch blocks, the array
    the receivers first .. last (A of them), bins [A, 2] int32 each receiver's window of bins b0, b1, observed [A, n_bins]
    float64 the observed envelope on the run's bins (amplitudes), weights the five component weights (>= 0), smooth_syn /
    smooth_obs the three-point passes over either row, max_lag the largest lag in bins, amplitude 1 to compare the roots of
    the energies.  Returns a dict of tensors, all WRITTEN: misfit [A, 6] (scale, rho, chi, peak-normalised distance, lag
    in bins, centroid distance in bins), misfit_se [A, 6] (with_se; default: B >= 2), xcorr and xcorr_se [A, 2 max_lag + 1]
    (with_xcorr), envelope [A, n_bins] (with_envelope), lit [A] (int32), bad and bad_observed [1] (int64).  include/r3d.h
    has the arithmetic.  Asynchronous on `stream` (a raw hipStream_t; None: torch's current one)."""
    import torch
    lib = _ffi.hip_lib()
    if batch_energy.dim() != 4 or batch_energy.shape[3] != _ffi.R3D_N_ENERGY or batch_energy.dtype != torch.float64:
        raise ValueError("batch_energy must be float64 [B, S, n_bins, 5]")
    if not batch_energy.is_cuda or not batch_energy.is_contiguous():
        raise ValueError("the blocks must be a contiguous tensor on a GPU")
    B, S, n_bins = (int(v) for v in batch_energy.shape[:3])
    dev = batch_energy.device
    A = int(last) - int(first) + 1
    if A < 1 or last >= S:
        raise ValueError("the array first .. last must lie within the blocks' seismometers")
    if tuple(bins.shape) != (A, 2) or bins.element_size() != 4 or bins.dtype.is_floating_point or bins.device != dev \
            or not bins.is_contiguous():
        raise ValueError("bins must be a contiguous 32-bit integer tensor [A, 2] on the blocks' GPU")
    if tuple(observed.shape) != (A, n_bins) or observed.dtype != torch.float64 or observed.device != dev \
            or not observed.is_contiguous():
        raise ValueError("observed must be a contiguous float64 tensor [A, n_bins] on the blocks' GPU")
    with_se = B >= 2 if with_se is None else with_se
    n_lags = 2 * int(max_lag) + 1

    def f64(*shape):
        return torch.empty(shape, dtype=torch.float64, device=dev)

    def i64():
        return torch.zeros(1, dtype=torch.int64, device=dev)
    out = dict(misfit=f64(A, _ffi.R3D_MISFIT_N), misfit_se=f64(A, _ffi.R3D_MISFIT_N) if with_se else None,
               xcorr=f64(A, n_lags) if with_xcorr else None, xcorr_se=f64(A, n_lags) if with_xcorr and with_se else None,
               envelope=f64(A, n_bins) if with_envelope else None, lit=torch.empty(A, dtype=torch.int32, device=dev),
               bad=i64(), bad_observed=i64())
    spec = misfit_spec(S, n_bins, first, last, weights, bins.data_ptr(), observed.data_ptr(), smooth_syn, smooth_obs, max_lag,
                       amplitude)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    ptr = {k: (v.data_ptr() if v is not None else None) for k, v in out.items()}
    rc = lib.r3d_envelope_misfit(dev.index or 0, B, batch_energy.data_ptr(), C.byref(spec), ptr["misfit"], ptr["misfit_se"],
                                 ptr["xcorr"], ptr["xcorr_se"], ptr["envelope"], ptr["lit"], ptr["bad"], ptr["bad_observed"],
                                 stream)
    if rc:
        raise RuntimeError("r3d_envelope_misfit failed: " + lib.r3d_last_error().decode())
    return out


def slant_shifts(dt, distances, r_ref, p0, dp, n_slowness):
    """r3d_slant_shifts (host only): the shifts of the slowness grid p0 + m dp (s/km) over receivers at `distances` (km) about
    r_ref, in bins of dt seconds.  Returns (shift_bin [M, A] int32, shift_frac [M, A] float64 in [0, 1))."""
    lib = _ffi.hip_lib()
    r = np.ascontiguousarray(distances, dtype=np.float64).reshape(-1)
    k = np.zeros((int(n_slowness), r.size), dtype=np.int32)
    f = np.zeros((int(n_slowness), r.size), dtype=np.float64)
    if lib.r3d_slant_shifts(float(dt), r.size, r.ctypes.data_as(_ffi._dp), float(r_ref), float(p0), float(dp), int(n_slowness),
                            k.ctypes.data_as(C.POINTER(C.c_int32)), f.ctypes.data_as(_ffi._dp)):
        raise ValueError(lib.r3d_last_error().decode())
    return k, f


def slant_spec(n_seismometers, n_bins, first, last, weights, shift_bin_ptr, shift_frac_ptr, gain_ptr, windows_ptr, n_slowness,
               n_windows, p0=0.0, dp=0.0, smooth=0, amplitude=1):
    """An r3d_slant_spec (include/r3d.h): the addresses of the int32 [M][A] and float64 [M][A] shifts, the float64 [A] gains
    and the uint32 [W][2] windows -- on the device for slant_stack, on the host for Engine.run_batched_slant_stack."""
    w = [float(v) for v in weights]
    if len(w) != _ffi.R3D_N_ENERGY:
        raise ValueError("five component weights (X, Y, Z, P, S) are needed")
    return _ffi.SlantSpec(size=C.sizeof(_ffi.SlantSpec), n_seismometers=int(n_seismometers), n_bins=int(n_bins), first=int(first),
                          last=int(last), smooth=int(smooth), amplitude=int(amplitude), n_slowness=int(n_slowness),
                          n_windows=int(n_windows), p0=float(p0), dp=float(dp), d_shift_bin=shift_bin_ptr,
                          d_shift_frac=shift_frac_ptr, d_gain=gain_ptr, d_windows=windows_ptr,
                          weight=(C.c_double * _ffi.R3D_N_ENERGY)(*w))


def slant_stack(batch_energy, shift_bin, shift_frac, gain, windows, first, last, weights, p0=0.0, dp=0.0, smooth=0, amplitude=1,
                with_se=None, stream=None):
    """r3d_slant_stack on torch tensors of one device: batch_energy [B, S, n_bins, 5] float64 are B batch blocks, the array the
    receivers first .. last (A of them), shift_bin [M, A] int32 and shift_frac [M, A] float64 the shifts of the M slownesses
    (slant_shifts makes them), gain [A] float64 the receivers' multipliers, windows [W, 2] int32 the delay windows c0, c1 (W may
    be 0), p0 and dp the slowness grid the picked slowness is expressed in.  Returns a dict of tensors, all WRITTEN: stack [M,
    n_bins], fold [M, n_bins] (int32), power [W, M], picks [W, 4] (Pmax, p*, tau* in bins, the peak), their _se (with_se;
    default: B >= 2), bad and bad_shifts [1] (int64).  include/r3d.h has the arithmetic.  Asynchronous on `stream` (a raw
    hipStream_t; None: torch's current one)."""
    import torch
    lib = _ffi.hip_lib()
    if batch_energy.dim() != 4 or batch_energy.shape[3] != _ffi.R3D_N_ENERGY or batch_energy.dtype != torch.float64:
        raise ValueError("batch_energy must be float64 [B, S, n_bins, 5]")
    if not batch_energy.is_cuda or not batch_energy.is_contiguous():
        raise ValueError("the blocks must be a contiguous tensor on a GPU")
    B, S, n_bins = (int(v) for v in batch_energy.shape[:3])
    dev = batch_energy.device
    A = int(last) - int(first) + 1
    if A < 1 or last >= S:
        raise ValueError("the array first .. last must lie within the blocks' seismometers")
    M = int(shift_bin.shape[0]) if shift_bin.dim() == 2 else 0
    W = int(windows.shape[0]) if windows is not None else 0

    def on_device(t, shape, what, floating):
        if tuple(t.shape) != shape or t.device != dev or not t.is_contiguous() or \
                (t.dtype != torch.float64 if floating else (t.element_size() != 4 or t.dtype.is_floating_point)):
            raise ValueError(f"{what} must be a contiguous {'float64' if floating else '32-bit integer'} tensor "
                             f"{list(shape)} on the blocks' GPU")
    on_device(shift_bin, (M, A), "shift_bin", False)
    on_device(shift_frac, (M, A), "shift_frac", True)
    on_device(gain, (A,), "gain", True)
    if W:
        on_device(windows, (W, 2), "windows", False)
    with_se = B >= 2 if with_se is None else with_se

    def f64(*shape):
        return torch.empty(shape, dtype=torch.float64, device=dev)

    def i64():
        return torch.zeros(1, dtype=torch.int64, device=dev)
    out = dict(stack=f64(M, n_bins), stack_se=f64(M, n_bins) if with_se else None,
               fold=torch.empty((M, n_bins), dtype=torch.int32, device=dev), power=f64(W, M), power_se=f64(W, M) if with_se else None,
               picks=f64(W, _ffi.R3D_SLANT_N), picks_se=f64(W, _ffi.R3D_SLANT_N) if with_se else None, bad=i64(), bad_shifts=i64())
    spec = slant_spec(S, n_bins, first, last, weights, shift_bin.data_ptr(), shift_frac.data_ptr(), gain.data_ptr(),
                      windows.data_ptr() if W else None, M, W, p0, dp, smooth, amplitude)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    ptr = [(v.data_ptr() if v is not None else None) for v in out.values()]
    rc = lib.r3d_slant_stack(dev.index or 0, B, batch_energy.data_ptr(), C.byref(spec), *ptr, stream)
    if rc:
        raise RuntimeError("r3d_slant_stack failed: " + lib.r3d_last_error().decode())
    return out


def contrast_gains(distances, r_ref, power):
    """r3d_contrast_gains (host only): gain [A] = (distances / r_ref)^power, the multipliers of a region's sums."""
    lib = _ffi.hip_lib()
    r = np.ascontiguousarray(distances, dtype=np.float64).reshape(-1)
    g = np.zeros(r.size)
    if lib.r3d_contrast_gains(r.size, r.ctypes.data_as(_ffi._dp), float(r_ref), float(power), g.ctypes.data_as(_ffi._dp)):
        raise ValueError(lib.r3d_last_error().decode())
    return g


def contrast_decibel(n_base, n_test, rho, loo=None):
    """r3d_contrast_decibel (host only): (dB, se) = 10 log10(rho) and the two-sample jackknife se of 10 log10 of the n_base +
    n_test leave-one-out quotients `loo` (array_contrast's region_loo[r][w]; None: no se); NaN where rho or a quotient is not
    positive."""
    lib = _ffi.hip_lib()
    q = None
    if loo is not None:
        q = np.ascontiguousarray(loo, dtype=np.float64).reshape(-1)
        if q.size != int(n_base) + int(n_test):
            raise ValueError("loo must hold n_base + n_test quotients")
    db, se = C.c_double(), C.c_double()
    if lib.r3d_contrast_decibel(int(n_base), int(n_test), float(rho), q.ctypes.data_as(_ffi._dp) if q is not None else None,
                                C.byref(db), C.byref(se)):
        raise ValueError(lib.r3d_last_error().decode())
    return db.value, se.value


def contrast_spec(n_seismometers, n_bins, first, last, weights, bins_ptr, gain_ptr, n_windows, regions=(), scale=(1.0, 1.0), smooth=0):
    """An r3d_contrast_spec (include/r3d.h): the addresses of the uint32 [A][W][2] bins and the float64 [A] gains -- on the
    device for array_contrast, on the host for Engine.run_batched_contrast; regions: (i0, i1) pairs, indices into the array."""
    w = [float(v) for v in weights]
    if len(w) != _ffi.R3D_N_ENERGY:
        raise ValueError("five component weights (X, Y, Z, P, S) are needed")
    reg = [(int(a), int(b)) for a, b in regions]
    spec = _ffi.ContrastSpec(size=C.sizeof(_ffi.ContrastSpec), n_seismometers=int(n_seismometers), n_bins=int(n_bins), first=int(first),
                             last=int(last), smooth=int(smooth), n_windows=int(n_windows), n_regions=len(reg), d_bins=bins_ptr,
                             d_gain=gain_ptr, weight=(C.c_double * _ffi.R3D_N_ENERGY)(*w), scale=(C.c_double * 2)(*[float(v) for v in scale]))
    for k, (a, b) in enumerate(reg[:_ffi.R3D_CONTRAST_MAX_REGIONS]):
        spec.regions[k][0], spec.regions[k][1] = a, b
    return spec


def array_contrast(base_energy, test_energy, first, last, weights, bins=None, regions=(), gain=None, scale=(1.0, 1.0), smooth=0,
                   with_se=None, stream=None):
    """r3d_array_contrast on torch tensors of one device: base_energy [Ba, S, n_bins, 5] and test_energy [Bb, S, n_bins, 5]
    float64 are the batch blocks of the two runs, the array the receivers first .. last (A of them), bins [A, W, 2] int32 each
    receiver's windows b0, b1 (None: no window), regions (i0, i1) pairs of array indices, gain [A] float64 the receivers'
    multipliers in a region's sums, scale the two sides' multipliers.  Returns a dict of tensors, all WRITTEN: contrast [A,
    n_bins], lit [A] (int32), window [A, W, 3] (Ea, Eb, rho), region [R, W, 3] (Na, Nb, rho_R), their _se and region_loo [R, W,
    Ba + Bb] (with_se; default: both B >= 2; else None), bad [1] (int64).  include/r3d.h has the arithmetic.  Asynchronous on
    `stream` (a raw hipStream_t; None: torch's current one)."""
    import torch
    lib = _ffi.hip_lib()
    for t in (base_energy, test_energy):
        if t.dim() != 4 or t.shape[3] != _ffi.R3D_N_ENERGY or t.dtype != torch.float64:
            raise ValueError("the blocks must be float64 [B, S, n_bins, 5]")
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("the blocks must be contiguous tensors on a GPU")
    if base_energy.device != test_energy.device or tuple(base_energy.shape[1:]) != tuple(test_energy.shape[1:]):
        raise ValueError("the two runs' blocks must lie on one GPU and have the same shape behind the batches")
    Ba, S, n_bins = (int(v) for v in base_energy.shape[:3])
    Bb = int(test_energy.shape[0])
    dev = base_energy.device
    A = int(last) - int(first) + 1
    if A < 1 or last >= S:
        raise ValueError("the array first .. last must lie within the blocks' seismometers")
    W = int(bins.shape[1]) if bins is not None else 0
    R = len(regions)
    if W and (tuple(bins.shape) != (A, W, 2) or bins.device != dev or not bins.is_contiguous() or bins.element_size() != 4 or
              bins.dtype.is_floating_point):
        raise ValueError("bins must be a contiguous 32-bit integer tensor [A, W, 2] on the blocks' GPU")
    if gain is not None and (tuple(gain.shape) != (A,) or gain.device != dev or not gain.is_contiguous() or gain.dtype != torch.float64):
        raise ValueError("gain must be a contiguous float64 tensor [A] on the blocks' GPU")
    with_se = (Ba >= 2 and Bb >= 2) if with_se is None else with_se

    def f64(*shape):
        return torch.empty(shape, dtype=torch.float64, device=dev)
    out = dict(contrast=f64(A, n_bins), contrast_se=f64(A, n_bins) if with_se else None,
               lit=torch.empty(A, dtype=torch.int32, device=dev), window=f64(A, W, _ffi.R3D_CONTRAST_N),
               window_se=f64(A, W, _ffi.R3D_CONTRAST_N) if with_se else None, region=f64(R, W, _ffi.R3D_CONTRAST_N),
               region_se=f64(R, W, _ffi.R3D_CONTRAST_N) if with_se else None, region_loo=f64(R, W, Ba + Bb) if with_se else None,
               bad=torch.zeros(1, dtype=torch.int64, device=dev))
    spec = contrast_spec(S, n_bins, first, last, weights, bins.data_ptr() if W else None, gain.data_ptr() if gain is not None else None,
                         W, regions, scale, smooth)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    ptr = [(v.data_ptr() if v is not None else None) for v in out.values()]
    rc = lib.r3d_array_contrast(dev.index or 0, Ba, base_energy.data_ptr(), Bb, test_energy.data_ptr(), C.byref(spec), *ptr, stream)
    if rc:
        raise RuntimeError("r3d_array_contrast failed: " + lib.r3d_last_error().decode())
    return out


def _check_blocks(blocks, lead, what):
    """[lead, ...] contiguous 8-byte tensors on one GPU, float64 first, 64-bit integers after it (None: skipped)."""
    import torch
    first = blocks[0]
    for k, t in enumerate(blocks):
        if t is None:
            continue
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != 8 or t.shape[0] != lead or t.device != first.device:
            raise ValueError(f"{what} must be contiguous 8-byte tensors [{lead}, ...] on one GPU")
        if (k == 0 and t.dtype != torch.float64) or (k > 0 and t.dtype.is_floating_point):
            raise ValueError(f"{what}: the energies are float64, counts and scalars 64-bit integers")


def batch_partial(batch_energy, batch_counts, batch_scalars=None, stream=None):
    """r3d_batch_partial on torch tensors of one device: a shard's half of a sharded job's standard errors.  The B batch
    blocks as for batch_moments; returns (energy_sum, energy_ss, counts_sum, counts_ss, scalars_sum) -- every entry's sum
    over the blocks and its sum of squared deviations from their mean (float64), scalars_sum None without
    batch_scalars.  batch_merge finishes from the states of all shards (include/r3d.h has the estimator).
    Asynchronous on `stream` (a raw hipStream_t; None: torch's current one)."""
    import torch
    lib = _ffi.hip_lib()
    B = int(batch_energy.shape[0])
    _check_blocks((batch_energy, batch_counts, batch_scalars), B, "batch blocks")
    dev = batch_energy.device
    ne, nc = batch_energy[0].numel(), batch_counts[0].numel()
    energy_sum = torch.empty(batch_energy.shape[1:], dtype=torch.float64, device=dev)
    energy_ss = torch.empty_like(energy_sum)
    counts_sum = torch.empty(batch_counts.shape[1:], dtype=batch_counts.dtype, device=dev)
    counts_ss = torch.empty(batch_counts.shape[1:], dtype=torch.float64, device=dev)
    scalars_sum = None
    if batch_scalars is not None:
        scalars_sum = torch.empty(batch_scalars.shape[1:], dtype=batch_scalars.dtype, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.r3d_batch_partial(dev.index or 0, B, batch_energy.data_ptr(), ne, batch_counts.data_ptr(), nc,
                               batch_scalars.data_ptr() if batch_scalars is not None else None,
                               batch_scalars[0].numel() if batch_scalars is not None else 0,
                               energy_sum.data_ptr(), energy_ss.data_ptr(), counts_sum.data_ptr(), counts_ss.data_ptr(),
                               scalars_sum.data_ptr() if scalars_sum is not None else None, stream)
    if rc:
        raise RuntimeError("r3d_batch_partial failed: " + lib.r3d_last_error().decode())
    return energy_sum, energy_ss, counts_sum, counts_ss, scalars_sum


def batch_merge(energy_sum, energy_ss, counts_sum, counts_ss, n_batches, scalars_sum=None, energy=None, counts=None,
                scalars=None, stream=None):
    """r3d_batch_merge on torch tensors of one device: the states of D shards, stacked [D, ...] in shard order (what
    batch_partial returned on each, n_batches blocks per shard), merged into the job's totals and the standard errors
    of its D * n_batches batches.  Returns (energy, counts, scalars, energy_se, counts_se) as batch_moments does: the
    totals ADDED into `energy` / `counts` / `scalars` (made and zeroed here when None).  Asynchronous on `stream`."""
    import torch
    lib = _ffi.hip_lib()
    D = int(energy_sum.shape[0])
    _check_blocks((energy_sum, counts_sum, scalars_sum), D, "shard sums")
    dev = energy_sum.device
    for t, like in ((energy_ss, energy_sum), (counts_ss, counts_sum)):
        if t.dtype != torch.float64 or t.shape != like.shape or t.device != dev or not t.is_contiguous():
            raise ValueError("the squared deviations must be contiguous float64 tensors shaped like their sums")
    if energy is None:
        energy = torch.zeros(energy_sum.shape[1:], dtype=torch.float64, device=dev)
    if counts is None:
        counts = torch.zeros(counts_sum.shape[1:], dtype=counts_sum.dtype, device=dev)
    if scalars is None and scalars_sum is not None:
        scalars = torch.zeros(scalars_sum.shape[1:], dtype=scalars_sum.dtype, device=dev)
    ne, nc = energy_sum[0].numel(), counts_sum[0].numel()
    for t, n in ((energy, ne), (counts, nc)):
        if t.device != dev or not t.is_contiguous() or t.numel() != n or t.element_size() != 8:
            raise ValueError("totals must be contiguous 8-byte tensors of a shard state's size on the states' GPU")
    energy_se = torch.empty(energy_sum.shape[1:], dtype=torch.float64, device=dev)
    counts_se = torch.empty(counts_sum.shape[1:], dtype=torch.float64, device=dev)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.r3d_batch_merge(dev.index or 0, D, int(n_batches), energy_sum.data_ptr(), energy_ss.data_ptr(), ne,
                             counts_sum.data_ptr(), counts_ss.data_ptr(), nc,
                             scalars_sum.data_ptr() if scalars_sum is not None else None,
                             scalars_sum[0].numel() if scalars_sum is not None else 0,
                             energy.data_ptr(), counts.data_ptr(), scalars.data_ptr() if scalars is not None else None,
                             energy_se.data_ptr(), counts_se.data_ptr(), stream)
    if rc:
        raise RuntimeError("r3d_batch_merge failed: " + lib.r3d_last_error().decode())
    return energy, counts, scalars, energy_se, counts_se


def precision_spec(n_seismometers, n_bins, first, last, bins=None, mask=_ffi.R3D_PRECISION_DEFAULT_MASK, min_count=16,
                   rel=0.1, coverage=0.9):
    """An r3d_precision_spec (include/r3d.h): the receivers first .. last (inclusive), the bins [bins[0], bins[1]) (None:
    all), the component mask over X, Y, Z, P, S (default P | S: an axis normal to the motion holds rounding noise and
    would keep any run from being met), and the target -- an entry of a bin with at least min_count arrivals is within
    when se <= rel * T, the run is met when the share `coverage` of the selected entries is.  The defaults are
    defaults, not measurements."""
    lo, hi = (0, n_bins) if bins is None else bins
    return _ffi.PrecisionSpec(C.sizeof(_ffi.PrecisionSpec), first, last, lo, hi, mask, n_seismometers, n_bins, min_count,
                              rel, coverage)


def precision_judge(energy, energy_se, counts, first, last, bins=None, mask=_ffi.R3D_PRECISION_DEFAULT_MASK, min_count=16,
                    rel=0.1, coverage=0.9, outputs=None, stream=None):
    """r3d_batch_precision on torch tensors of one device: energy, energy_se [S, n_bins, 5] float64 and counts
    [S, n_bins, 2] of a 64-bit integer type, judged against precision_spec(...) where they lie.  Returns (per_receiver
    [last - first + 1, 3] int64 -- selected, within, zero --, worst_per_receiver [last - first + 1], totals [3] int64,
    worst [1]) on the device; `outputs` gives the four tensors instead (rows beyond the selected receivers are left
    alone).  Asynchronous on `stream` (a raw hipStream_t; None: torch's current one)."""
    import torch
    lib = _ffi.hip_lib()
    dev = energy.device
    if energy.dim() != 3 or energy.shape[2] != _ffi.R3D_N_ENERGY or energy.dtype != torch.float64 or not energy.is_cuda:
        raise ValueError("energy must be a float64 tensor [S, n_bins, 5] on a GPU")
    S, nb = int(energy.shape[0]), int(energy.shape[1])
    if energy_se.shape != energy.shape or energy_se.dtype != torch.float64 or energy_se.device != dev:
        raise ValueError("energy_se must be shaped like energy, float64, on its GPU")
    if tuple(counts.shape) != (S, nb, _ffi.R3D_N_COUNT) or counts.element_size() != 8 or counts.dtype.is_floating_point or \
            counts.device != dev:
        raise ValueError("counts must be a 64-bit integer tensor [S, n_bins, 2] on the energies' GPU")
    if not (energy.is_contiguous() and energy_se.is_contiguous() and counts.is_contiguous()):
        raise ValueError("the three arrays must be contiguous")
    spec = precision_spec(S, nb, first, last, bins, mask, min_count, rel, coverage)
    A = max(int(last) - int(first) + 1, 1)
    if outputs is None:
        outputs = (torch.zeros((A, 3), dtype=torch.int64, device=dev), torch.zeros(A, dtype=torch.float64, device=dev),
                   torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev))
    rows, worst_rows, totals, worst = outputs
    for t, n in ((rows, 3 * A), (worst_rows, A), (totals, 3), (worst, 1)):
        if t.device != dev or not t.is_contiguous() or t.numel() < n or t.element_size() != 8:
            raise ValueError("outputs must be contiguous 8-byte tensors of at least the selected receivers' size on the GPU")
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    if lib.r3d_batch_precision(dev.index or 0, energy.data_ptr(), energy_se.data_ptr(), counts.data_ptr(), S, nb,
                               C.byref(spec), rows.data_ptr(), worst_rows.data_ptr(), totals.data_ptr(), worst.data_ptr(),
                               stream):
        raise RuntimeError("r3d_batch_precision failed: " + lib.r3d_last_error().decode())
    return rows, worst_rows, totals, worst


def run_model(model, n, first_id=0, seed=0x5EED, n_gpus=1, devices=None):
    """r3d_run_model: the whole seam in one call, sharded over devices 0 .. n_gpus-1 -- or, with
    `devices`, r3d_run_model_on: shard g on devices[g] (a device may be named more than once)."""
    lib = _ffi.hip_lib()
    res = model.new_result()
    c = res._as_c()
    if devices is not None:
        devs = (C.c_int * len(devices))(*devices)
        rc = lib.r3d_run_model_on(model.desc_p, n, first_id, seed, devs, len(devices), C.byref(c))
    else:
        rc = lib.r3d_run_model(model.desc_p, n, first_id, seed, n_gpus, C.byref(c))
    if rc:
        raise RuntimeError("r3d_run_model failed: " + lib.r3d_last_error().decode())
    res._from_c(c)
    return res


def _run_batched_to_host(lib, name, handle, model, n, first_id, seed, n_batches, result, *tail):
    """What the calls that bring a batched run to the host share: `name` of `lib` on `handle` with the totals ADDED
    into `result` (a new one when None) and the two standard-error arrays written, `tail` the call's own arguments
    behind those.  Returns (Result, energy_se, counts_se)."""
    res = result if result is not None else model.new_result()
    shape = (model.n_seismometers, model.n_bins)
    ese, cse = np.zeros(shape + (_ffi.R3D_N_ENERGY,)), np.zeros(shape + (_ffi.R3D_N_COUNT,))
    c = res._as_c()
    if getattr(lib, name)(handle, n, first_id, seed, n_batches, C.byref(c), ese.ctypes.data_as(_ffi._dp),
                          cse.ctypes.data_as(_ffi._dp), *tail):
        raise RuntimeError(name + " failed: " + lib.r3d_last_error().decode())
    res._from_c(c)
    return res, ese, cse


class Node:
    """r3d_node_*: one engine per entry of `devices`, kept across runs; a run shards the id range over them
    and sums the shards' blocks on the devices (RCCL ncclReduce to devices[0]; on the host for a node of one
    shard, when two shards share a device or when RCCL is not to be had -- `reduction` says which,
    `reduction_note` why)."""

    def __init__(self, model, devices, lib=None):
        self.model = model
        self._lib = _ffi.hip_lib(path=lib)
        devs = (C.c_int * len(devices))(*devices)
        self._n = self._lib.r3d_node_create(model.desc_p, devs, len(devices))
        if not self._n:
            raise RuntimeError("r3d_node_create failed: " + self._lib.r3d_last_error().decode())

    @property
    def reduction(self):
        return self._lib.r3d_node_reduction(self._n).decode()

    @property
    def reduction_note(self):
        """Why the host adds the shards' blocks, when it does (r3d_node_reduction_note)."""
        return self._lib.r3d_node_reduction_note(self._n).decode()

    def __len__(self):
        return self._lib.r3d_node_size(self._n)

    def run(self, n, first_id=0, seed=0x5EED, result=None):
        res = result if result is not None else self.model.new_result()
        c = res._as_c()
        if self._lib.r3d_node_run(self._n, n, first_id, seed, C.byref(c)):
            raise RuntimeError("r3d_node_run failed: " + self._lib.r3d_last_error().decode())
        res._from_c(c)
        return res

    def run_batched(self, n, n_batches, first_id=0, seed=0x5EED, result=None):
        """r3d_node_run_batched: the job's ids as n_batches id-partitioned batches, n_batches / len(self) (2..64) of
        them on every shard; the shards' moments are merged on the GPU.  Returns (Result, energy_se, counts_se) as
        Engine.run_batched does -- the job's totals (ADDED into `result` when one is given) and the standard error of
        every energy and count entry from the spread of all n_batches batches."""
        return _run_batched_to_host(self._lib, "r3d_node_run_batched", self._n, self.model, n, first_id, seed, n_batches,
                                    result)

    def engine(self, shard):
        """r3d_node_engine: shard g's engine as a raw handle for the library's calls (it stays the node's)."""
        e = self._lib.r3d_node_engine(self._n, int(shard))
        if not e:
            raise IndexError(shard)
        return e

    def close(self):
        if self._n:
            self._lib.r3d_node_destroy(self._n)
            self._n = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def reduce_volumes_by_frame(engines):
    """r3d_volume_reduce_by_frame: the grids of several engines of ONE process (one per shard of a job, each
    with its own grid of the same shape, on any devices) added by frame; engine g ends with the job's counts
    for frames [frames[g], frames[g + 1]).  Returns (frames, saturated cells)."""
    lib = engines[0]._lib
    n = len(engines)
    handles = (C.c_void_p * n)(*[e._e for e in engines])
    frames = (C.c_uint32 * (n + 1))()
    sat = C.c_uint64(0)
    if lib.r3d_volume_reduce_by_frame(handles, n, frames, C.byref(sat)):
        raise RuntimeError("r3d_volume_reduce_by_frame failed: " + lib.r3d_last_error().decode())
    return list(frames), int(sat.value)


def volume_desc(origin, cell_size, dims, n_frames, frame_dt):
    v = _ffi.VolumeDesc()
    for k in range(3):
        v.origin[k], v.cell_size[k], v.dims[k] = origin[k], cell_size[k], dims[k]
    v.n_frames, v.frame_dt = n_frames, frame_dt
    return v


def range_bins(desc, epicentre, dr, n_range, azimuth_deg=0.0, half_width_deg=180.0):
    """r3d_volume_range_bins: the column map of the elevation view, numpy uint32 [ny][nx] -- the range bin
    floor(rho / dr) of every column's centre, rho its horizontal distance from `epicentre` (x, y), or 0xFFFFFFFF
    for a column beyond n_range bins or outside azimuth_deg +- half_width_deg (half_width_deg >= 180: no filter).
    `desc`: a volume_desc(...).  Made on the host; needs no GPU.  include/r3d.h has the definition."""
    lib = _ffi.hip_lib()
    out = np.empty((int(desc.dims[1]), int(desc.dims[0])), dtype=np.uint32)
    epi = (C.c_double * 2)(float(epicentre[0]), float(epicentre[1]))
    if lib.r3d_volume_range_bins(C.byref(desc), epi, float(dr), int(n_range), float(azimuth_deg), float(half_width_deg),
                                 out.ctypes.data_as(C.POINTER(C.c_uint32))):
        raise RuntimeError("r3d_volume_range_bins failed: " + lib.r3d_last_error().decode())
    return out


def _grid_shape(counters, desc):
    """(nx, ny, nz, device) of a grid tensor, held against its description (a volume_desc)."""
    if not counters.is_cuda or not counters.is_contiguous() or counters.element_size() != 4:
        raise ValueError("the grid must be a contiguous tensor of 32-bit counters on a GPU")
    nx, ny, nz = (int(d) for d in desc.dims)
    if counters.numel() != 2 * int(desc.n_frames) * nz * ny * nx:
        raise ValueError("the grid does not have the description's size")
    return nx, ny, nz, counters.device


def project_volume(counters, desc, frame_begin, frame_end, frame_group=1, range_bin=None, n_range=0, above=True,
                   outputs=None, stream=None):
    """r3d_volume_project on torch tensors: `counters` is a grid of the shape `desc` (a volume_desc) on a GPU, 32-bit.
    Returns (above, elev, outside): int64 device tensors [2][n_out][ny][nx], [2][n_out][nz][n_range] and [2] holding
    the uint64 sums (above is None with above=False; elev and outside are None without a `range_bin` map -- a
    uint32 [ny][nx] numpy array from range_bins(), or a 32-bit tensor already on the device).  `outputs`: the same
    triple from an earlier call, to be ADDED into.  Asynchronous on `stream` (a raw hipStream_t; None: torch's
    current one).  include/r3d.h has the definition of the views."""
    import torch
    lib = _ffi.hip_lib()
    nx, ny, nz, dev = _grid_shape(counters, desc)
    n_out = max(0, -(-(int(frame_end) - int(frame_begin)) // max(1, int(frame_group))))
    elev_on = range_bin is not None
    if elev_on and not torch.is_tensor(range_bin):
        range_bin = torch.from_numpy(np.ascontiguousarray(range_bin, dtype=np.uint32).view(np.int32)).to(dev)
    if elev_on and (range_bin.device != dev or range_bin.numel() != ny * nx or range_bin.element_size() != 4
                    or not range_bin.is_contiguous()):
        raise ValueError("range_bin must be [ny][nx] contiguous 32-bit values on the grid's GPU")
    a, e, o = outputs if outputs is not None else (None, None, None)
    if (not above and a is not None) or (not elev_on and (e is not None or o is not None)):
        raise ValueError("`outputs` holds a view that this call does not ask for")
    if above and a is None:
        a = torch.zeros((2, n_out, ny, nx), dtype=torch.int64, device=dev)
    if elev_on and e is None:
        e = torch.zeros((2, n_out, nz, int(n_range)), dtype=torch.int64, device=dev)
    if elev_on and o is None:
        o = torch.zeros(2, dtype=torch.int64, device=dev)
    for t, shape in ((a, (2, n_out, ny, nx)), (e, (2, n_out, nz, int(n_range))), (o, (2,))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.int64 or t.device != dev or not t.is_contiguous()):
            raise ValueError(f"a view to add into must be a contiguous int64 tensor {shape} on the grid's GPU")
    views = _ffi.VolumeViews(size=C.sizeof(_ffi.VolumeViews), frame_begin=int(frame_begin), frame_end=int(frame_end),
                             frame_group=int(frame_group), n_range=int(n_range) if elev_on else 0,
                             d_range_bin=range_bin.data_ptr() if elev_on else None,
                             d_above=a.data_ptr() if a is not None else None,
                             d_elev=e.data_ptr() if e is not None else None,
                             d_outside=o.data_ptr() if o is not None else None)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    if lib.r3d_volume_project(dev.index or 0, counters.data_ptr(), C.byref(desc), C.byref(views), stream):
        raise RuntimeError("r3d_volume_project failed: " + lib.r3d_last_error().decode())
    return a, e, o


def neutral_time_maps(desc, device, first=True, peak=True, total=True):
    """The maps of time_maps_volume in their neutral state (include/r3d.h): (first, peak_frame, peak_count, total), int32
    device tensors [2][nz][ny][nx] holding uint32 bits -- first and peak_frame all 0xFFFFFFFF, peak_count 0 -- and an
    int64 one for total, 0; None for a map not asked for."""
    import torch
    nx, ny, nz = (int(d) for d in desc.dims)
    shape = (2, nz, ny, nx)
    never = lambda: torch.full(shape, -1, dtype=torch.int32, device=device)   # noqa: E731
    return (never() if first else None, never() if peak else None,
            torch.zeros(shape, dtype=torch.int32, device=device) if peak else None,
            torch.zeros(shape, dtype=torch.int64, device=device) if total else None)


def time_maps_volume(counters, desc, frame_begin, frame_end, min_count=1, first=True, peak=True, total=True, outputs=None,
                     stream=None):
    """r3d_volume_time_maps on torch tensors: `counters` is a grid of the shape `desc` (a volume_desc) on a GPU, 32-bit.
    Returns (first, peak_frame, peak_count, total) as neutral_time_maps() makes them, UPDATED with the frames
    [frame_begin, frame_end): the first frame with min_count events, the frame and count of the peak, the sum (a map
    not asked for is None).  `outputs`: the same four from an earlier call, to be brought up to date with this call's
    frames; frames are absolute, pieces of a range in any order give the maps of one call.  Asynchronous on `stream`
    (a raw hipStream_t; None: torch's current one).  include/r3d.h has the definition."""
    import torch
    lib = _ffi.hip_lib()
    nx, ny, nz, dev = _grid_shape(counters, desc)
    if outputs is None:
        outputs = neutral_time_maps(desc, dev, first, peak, total)
    fi, pf, pc, to = outputs
    if (not first and fi is not None) or (not peak and (pf is not None or pc is not None)) or (not total and to is not None):
        raise ValueError("`outputs` holds a map that this call does not ask for")
    for t, dtype in ((fi, torch.int32), (pf, torch.int32), (pc, torch.int32), (to, torch.int64)):
        if t is not None and (tuple(t.shape) != (2, nz, ny, nx) or t.dtype != dtype or t.device != dev or not t.is_contiguous()):
            raise ValueError(f"a map to update must be a contiguous {dtype} tensor {(2, nz, ny, nx)} on the grid's GPU")
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    maps = _ffi.VolumeMaps(size=C.sizeof(_ffi.VolumeMaps), frame_begin=int(frame_begin), frame_end=int(frame_end),
                           min_count=int(min_count), d_first=ptr(fi), d_peak_frame=ptr(pf), d_peak_count=ptr(pc),
                           d_total=ptr(to))
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    if lib.r3d_volume_time_maps(dev.index or 0, counters.data_ptr(), C.byref(desc), C.byref(maps), stream):
        raise RuntimeError("r3d_volume_time_maps failed: " + lib.r3d_last_error().decode())
    return fi, pf, pc, to


class Engine:
    """The model resident in HBM + the HIP traversal kernels (libr3d_hip.so)."""

    def __init__(self, model, device=0, reproducible=False, lib=None, residency=None, pool_slots=None,
                 accumulator_bits=None, lds_reserve=None):
        """reproducible: the build without wave-voted series choices (see _ffi.hip_lib); lib: the path
        of another build of the engine (tools/).  residency, pool_slots, accumulator_bits, lds_reserve:
        the kernel's LDS carve-up in the caller's hands (include/r3d.h r3d_engine_opts) -- how the
        tests reach every compiled kernel variant on small models; None = automatic, and with all
        four None the engine is made by plain r3d_engine_create."""
        self._lib = _ffi.hip_lib(reproducible, lib)
        self.model = model
        self.device = int(device)
        self._volume_keepalive = None
        if residency is None and pool_slots is None and accumulator_bits is None and lds_reserve is None:
            self._e = self._lib.r3d_engine_create(model.desc_p, device)
        else:
            o = _ffi.EngineOpts(C.sizeof(_ffi.EngineOpts), -1 if residency is None else residency,
                                pool_slots or 0, -1 if accumulator_bits is None else accumulator_bits,
                                lds_reserve or 0)
            self._e = self._lib.r3d_engine_create_ex(model.desc_p, device, C.byref(o))
        if not self._e:
            raise RuntimeError("r3d_engine_create failed: " + self._lib.r3d_last_error().decode())
        if model.device_tables:   # mean free paths / dipoles are the engine's output
            for s in range(model.n_scatterers):
                st = self.scatterer_stats(s)
                model._lib.r3dh_model_set_scatterer_stats(model._h, s, (C.c_double * 2)(*st[0:2]),
                                                          (C.c_double * 2)(*st[2:4]))

    def close(self, discard_carried=False):
        """Release the engine.  Refuses (RuntimeError) while histories carried over by
        run_device(carry="carry") await their flush -- their tallies and bins would be lost --
        unless discard_carried is set."""
        if getattr(self, "_e", None):
            if discard_carried or self._lib.r3d_engine_close(self._e):
                if not discard_carried:
                    raise RuntimeError("r3d_engine_close failed: " + self._lib.r3d_last_error().decode())
                self._lib.r3d_engine_destroy(self._e)
            self._e = None
            self._volume_keepalive = None   # (only now may a caller-owned grid be freed)

    def __del__(self):
        try:
            self.close(discard_carried=True)
        except Exception:
            pass

    @property
    def carry_pending(self):
        return bool(self._lib.r3d_engine_carry_pending(self._e))

    def run(self, n, first_id=0, seed=0x5EED, result=None, trace=False):
        """Run histories [first_id, first_id+n); accumulate into `result`."""
        res = result if result is not None else self.model.new_result()
        c = res._as_c()
        finals = None
        if trace:
            finals = (_ffi.Final * n)()
            rc = self._lib.r3d_run_traced(self._e, n, first_id, seed, C.byref(c), finals)
        else:
            rc = self._lib.r3d_run(self._e, n, first_id, seed, C.byref(c))
        if rc:
            raise RuntimeError("r3d_run failed: " + self._lib.r3d_last_error().decode())
        res._from_c(c)
        return (res, finals) if trace else res

    def run_batched(self, n, n_batches, first_id=0, seed=0x5EED, keep_batches=False):
        """Histories [first_id, first_id+n) as n_batches id-partitioned batches (2..64), each a self-contained launch
        into its own block, overlapped on the library's streams: (Result, energy_se, counts_se) -- the run's totals
        as Engine.run gives them (to summation order) and the standard error of every energy and count entry from
        the spread of the batches (include/r3d.h r3d_run_batched; numpy arrays shaped like Result.energy / .counts).
        keep_batches: the run goes through r3d_run_device_batched on torch tensors and the blocks themselves follow
        as numpy arrays, (..., batch_energy[B, seis, bin, 5], batch_counts[B, seis, bin, 2])."""
        m = self.model
        if not keep_batches:
            return _run_batched_to_host(self._lib, "r3d_run_batched", self._e, m, n, first_id, seed, n_batches, None)
        res = m.new_result()
        shape = (m.n_seismometers, m.n_bins)
        import torch
        dev = torch.device("cuda", self.device)
        B = max(int(n_batches), 0)
        energy = torch.zeros(shape + (_ffi.R3D_N_ENERGY,), dtype=torch.float64, device=dev)
        counts = torch.zeros(shape + (_ffi.R3D_N_COUNT,), dtype=torch.int64, device=dev)
        scalars = torch.zeros(_ffi.R3D_N_SCALARS, dtype=torch.int64, device=dev)
        ese, cse = torch.zeros_like(energy), torch.zeros(counts.shape, dtype=torch.float64, device=dev)
        be = torch.zeros((B,) + tuple(energy.shape), dtype=torch.float64, device=dev)
        bc = torch.zeros((B,) + tuple(counts.shape), dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev)
        if self._lib.r3d_run_device_batched(self._e, n, first_id, seed, n_batches, energy.data_ptr(), counts.data_ptr(),
                                            scalars.data_ptr(), ese.data_ptr(), cse.data_ptr(), be.data_ptr(),
                                            bc.data_ptr(), stream.cuda_stream):
            raise RuntimeError("r3d_run_device_batched failed: " + self._lib.r3d_last_error().decode())
        stream.synchronize()
        res.energy[:] = energy.cpu().numpy()
        res.counts[:] = counts.cpu().numpy().view(np.uint64)
        res.set_scalars(scalars.cpu().numpy().view(np.uint64))
        return res, ese.cpu().numpy(), cse.cpu().numpy(), be.cpu().numpy(), bc.cpu().numpy().view(np.uint64)

    def run_to_precision(self, n_max, n_batches, rounds, first, last, bins=None, mask=_ffi.R3D_PRECISION_DEFAULT_MASK,
                         min_count=16, rel=0.1, coverage=0.9, first_id=0, seed=0x5EED, result=None):
        """r3d_run_to_precision: at most n_max histories in `rounds` rounds of n_max / rounds, each n_batches batches,
        judged on the GPU after every round against precision_spec(first, last, bins, mask, min_count, rel, coverage);
        the run stops at the first round that is met.  Returns (Result, energy_se, counts_se, report): what
        Node.run_batched gives for the rounds run as shards (the totals ADDED into `result` when one is given), and
        report = {rounds, histories, met, round_histories, n_selected, n_within, n_zero, worst -- one entry per round
        run --, per_receiver [last - first + 1, 3] (selected, within, zero) and worst_per_receiver of the last round}."""
        m = self.model
        res = result if result is not None else m.new_result()
        shape = (m.n_seismometers, m.n_bins)
        ese, cse = np.zeros(shape + (_ffi.R3D_N_ENERGY,)), np.zeros(shape + (_ffi.R3D_N_COUNT,))
        spec = precision_spec(m.n_seismometers, m.n_bins, first, last, bins, mask, min_count, rel, coverage)
        A = max(int(last) - int(first) + 1, 1)
        rows, worst_rows = np.zeros((A, 3), dtype=np.uint64), np.zeros(A)
        rep = _ffi.PrecisionReport()
        rep.size = C.sizeof(rep)
        rep.per_receiver, rep.worst_per_receiver = rows.ctypes.data, worst_rows.ctypes.data
        c = res._as_c()
        if self._lib.r3d_run_to_precision(self._e, n_max, first_id, seed, n_batches, rounds, C.byref(spec), C.byref(c),
                                          ese.ctypes.data_as(_ffi._dp), cse.ctypes.data_as(_ffi._dp), C.byref(rep)):
            raise RuntimeError("r3d_run_to_precision failed: " + self._lib.r3d_last_error().decode())
        res._from_c(c)
        G = rep.rounds
        report = {"rounds": G, "histories": rep.histories, "met": bool(rep.met),
                  "round_histories": np.array(rep.round_histories[:G], dtype=np.uint64),
                  "n_selected": np.array(rep.n_selected[:G], dtype=np.uint64),
                  "n_within": np.array(rep.n_within[:G], dtype=np.uint64),
                  "n_zero": np.array(rep.n_zero[:G], dtype=np.uint64), "worst": np.array(rep.worst[:G], dtype=np.float64),
                  "per_receiver": rows, "worst_per_receiver": worst_rows}
        return res, ese, cse, report

    def run_batched_windows(self, n, n_batches, bins, weights, first_id=0, seed=0x5EED, keep_batch_windows=False):
        """run_batched that also sums lapse windows where the batch blocks lie (include/r3d.h r3d_run_batched_windows):
        bins [S, W, 2] begin, end pairs (host; anything numpy makes uint32 of), weights the five component weights.
        Returns (Result, energy_se, counts_se, window_energy [S, W], window_counts [S, W, 2], window_se [S, W]) and,
        with keep_batch_windows, the batches' own window sums [B, S, W] behind them (window_log_ratio's input)."""
        m = self.model
        b = np.ascontiguousarray(bins, dtype=np.uint32)
        if b.ndim != 3 or b.shape[0] != m.n_seismometers or b.shape[2] != 2:
            raise ValueError("bins must be [n_seismometers, W, 2]")
        W = b.shape[1]
        spec = window_spec(m.n_seismometers, m.n_bins, W, b.ctypes.data, weights)
        we, wse = np.zeros((m.n_seismometers, W)), np.zeros((m.n_seismometers, W))
        wc = np.zeros((m.n_seismometers, W, _ffi.R3D_N_COUNT), dtype=np.uint64)
        bwe = np.zeros((max(int(n_batches), 0), m.n_seismometers, W)) if keep_batch_windows else None
        res, ese, cse = _run_batched_to_host(
            self._lib, "r3d_run_batched_windows", self._e, m, n, first_id, seed, n_batches, None, C.byref(spec),
            we.ctypes.data_as(_ffi._dp), wc.ctypes.data_as(C.POINTER(C.c_uint64)), wse.ctypes.data_as(_ffi._dp),
            bwe.ctypes.data_as(_ffi._dp) if bwe is not None else None)
        return (res, ese, cse, we, wc, wse) + ((bwe,) if keep_batch_windows else ())

    def run_batched_array_image(self, n, n_batches, first, last, weights, gamma_log2=1, rho=0.3, fit=(0, 0),
                                ranges=(0.0, 0.0), curve=(math.nan, math.nan), first_id=0, seed=0x5EED, keep_row_sums=False):
        """run_batched that also makes the travel-time image of the receivers first .. last where the batch blocks lie
        (include/r3d.h r3d_run_batched_array_image): weights the five component weights, gamma = 2^gamma_log2, rho the
        norm ratio; fit the 1-based (IBEGIN, IEND) of the power-law fit with `ranges` the distances of the two end
        receivers (Model.ttimage_plan), curve a (c, q) given outright.  Returns (Result, energy_se, counts_se, image): a
        dict of image, image_se [A, n_bins], lit, peak_bin [A] (uint32), summed, summed_se, peak [A] -- summed is the raw
        sum of bins --, with keep_row_sums batch_row_sum [B, A], and with a fit: fit (c, q), fit_se (se(ln c), se(q)),
        curve_made, curve [A], image_curve, image_curve_se [A, n_bins]."""
        m = self.model
        A = int(last) - int(first) + 1
        if A < 1:
            raise ValueError("the array needs first <= last")
        spec = array_image_spec(m.n_seismometers, m.n_bins, first, last, weights, gamma_log2, rho, None,
                                m.n_bins * m.desc.params.time_per_bin, fit, ranges, curve)
        img = dict(image=np.zeros((A, m.n_bins)), image_se=np.zeros((A, m.n_bins)), summed=np.zeros(A), summed_se=np.zeros(A),
                   peak=np.zeros(A), peak_bin=np.zeros(A, dtype=np.uint32), lit=np.zeros(A, dtype=np.uint32))
        if keep_row_sums:
            img["batch_row_sum"] = np.zeros((max(int(n_batches), 0), A))
        has_fit = bool(fit[0] or fit[1])
        if has_fit:
            img.update(curve=np.zeros(A), image_curve=np.zeros((A, m.n_bins)), image_curve_se=np.zeros((A, m.n_bins)))
        out = _ffi.ArrayImageResult(size=C.sizeof(_ffi.ArrayImageResult), **{k: v.ctypes.data for k, v in img.items()})
        res, ese, cse = _run_batched_to_host(self._lib, "r3d_run_batched_array_image", self._e, m, n, first_id, seed, n_batches,
                                             None, C.byref(spec), C.byref(out))
        if has_fit:
            img.update(fit=tuple(out.fit), fit_se=tuple(out.fit_se), curve_made=bool(out.curve_made))
        return res, ese, cse, img

    def run_batched_envelope_shape(self, n, n_batches, bins, first, last, weights, smooth=8, first_id=0, seed=0x5EED):
        """run_batched that also makes the envelope shape of the receivers first .. last where the batch blocks lie
        (include/r3d.h r3d_run_batched_envelope_shape): bins [A, 2] each receiver's window b0, b1 (host; Model.envshape_plan
        makes them), weights the five component weights, smooth the three-point passes.  Returns (Result, energy_se,
        counts_se, shape): a dict of shape, shape_se [A, 6], envelope, envelope_se [A, n_bins], peak_bin, half_bin, lit [A]
        (uint32; 0xFFFFFFFF: dead / undecayed)."""
        m = self.model
        A = int(last) - int(first) + 1
        if A < 1:
            raise ValueError("the array needs first <= last")
        b = np.ascontiguousarray(bins, dtype=np.uint32)
        if b.shape != (A, 2):
            raise ValueError("bins must be [A, 2]")
        spec = envelope_spec(m.n_seismometers, m.n_bins, first, last, weights, smooth, b.ctypes.data)
        shp = dict(shape=np.zeros((A, _ffi.R3D_ENVELOPE_N_SHAPE)), shape_se=np.zeros((A, _ffi.R3D_ENVELOPE_N_SHAPE)),
                   envelope=np.zeros((A, m.n_bins)), envelope_se=np.zeros((A, m.n_bins)), peak_bin=np.zeros(A, dtype=np.uint32),
                   half_bin=np.zeros(A, dtype=np.uint32), lit=np.zeros(A, dtype=np.uint32))
        out = _ffi.EnvelopeResult(size=C.sizeof(_ffi.EnvelopeResult), **{k: v.ctypes.data for k, v in shp.items()})
        res, ese, cse = _run_batched_to_host(self._lib, "r3d_run_batched_envelope_shape", self._e, m, n, first_id, seed,
                                             n_batches, None, C.byref(spec), C.byref(out))
        return res, ese, cse, shp

    def run_batched_envelope_bands(self, n, n_batches, bins, first, last, weights, smooth=8, n_replicates=1000, tail=50,
                                   bands_seed=0xB007, first_id=0, seed=0x5EED):
        """run_batched that also makes the bootstrap percentile bands of the receivers first .. last where the batch blocks
        lie (include/r3d.h r3d_run_batched_envelope_bands): bins [A, 2] each receiver's window b0, b1 (host;
        Model.envbands_plan or Model.envshape_plan makes them), weights the five component weights, smooth the three-point
        passes, n_replicates resamples by the counts of bands_seed, tail values outside either band.  Returns (Result,
        energy_se, counts_se, bands): a dict of envelope, envelope_lo, envelope_hi [A, n_bins], shape, shape_lo, shape_hi [A,
        6] and defined [A, 6] (uint32)."""
        m = self.model
        A = int(last) - int(first) + 1
        if A < 1:
            raise ValueError("the array needs first <= last")
        b = np.ascontiguousarray(bins, dtype=np.uint32)
        if b.shape != (A, 2):
            raise ValueError("bins must be [A, 2]")
        spec = bands_spec(m.n_seismometers, m.n_bins, first, last, weights, smooth, n_replicates, tail, bands_seed, b.ctypes.data)
        six = _ffi.R3D_ENVELOPE_N_SHAPE
        bands = dict(envelope=np.zeros((A, m.n_bins)), envelope_lo=np.zeros((A, m.n_bins)), envelope_hi=np.zeros((A, m.n_bins)),
                     shape=np.zeros((A, six)), shape_lo=np.zeros((A, six)), shape_hi=np.zeros((A, six)),
                     defined=np.zeros((A, six), dtype=np.uint32))
        out = _ffi.BandsResult(size=C.sizeof(_ffi.BandsResult), **{k: v.ctypes.data for k, v in bands.items()})
        res, ese, cse = _run_batched_to_host(self._lib, "r3d_run_batched_envelope_bands", self._e, m, n, first_id, seed,
                                             n_batches, None, C.byref(spec), C.byref(out))
        return res, ese, cse, bands

    def run_batched_envelope_misfit(self, n, n_batches, bins, observed, first, last, weights, smooth_syn=8, smooth_obs=0,
                                    max_lag=0, amplitude=1, first_id=0, seed=0x5EED):
        """run_batched that also makes the envelope misfit of the receivers first .. last against `observed` where the batch
        blocks lie (include/r3d.h r3d_run_batched_envelope_misfit): bins [A, 2] each receiver's window b0, b1 and observed
        [A, n_bins] the observed amplitudes on the run's bins (host; Model.envfit_plan makes both).  Returns (Result,
        energy_se, counts_se, fit): a dict of misfit, misfit_se [A, 6], xcorr, xcorr_se [A, 2 max_lag + 1], envelope [A,
        n_bins] and lit [A] (uint32)."""
        m = self.model
        A = int(last) - int(first) + 1
        if A < 1:
            raise ValueError("the array needs first <= last")
        b = np.ascontiguousarray(bins, dtype=np.uint32)
        o = np.ascontiguousarray(observed, dtype=np.float64)
        if b.shape != (A, 2) or o.shape != (A, m.n_bins):
            raise ValueError("bins must be [A, 2] and observed [A, n_bins]")
        spec = misfit_spec(m.n_seismometers, m.n_bins, first, last, weights, b.ctypes.data, o.ctypes.data, smooth_syn, smooth_obs,
                           max_lag, amplitude)
        n_lags = 2 * int(max_lag) + 1
        fit = dict(misfit=np.zeros((A, _ffi.R3D_MISFIT_N)), misfit_se=np.zeros((A, _ffi.R3D_MISFIT_N)), xcorr=np.zeros((A, n_lags)),
                   xcorr_se=np.zeros((A, n_lags)), envelope=np.zeros((A, m.n_bins)), lit=np.zeros(A, dtype=np.uint32))
        out = _ffi.MisfitResult(size=C.sizeof(_ffi.MisfitResult), **{k: v.ctypes.data for k, v in fit.items()})
        res, ese, cse = _run_batched_to_host(self._lib, "r3d_run_batched_envelope_misfit", self._e, m, n, first_id, seed,
                                             n_batches, None, C.byref(spec), C.byref(out))
        return res, ese, cse, fit

    def run_batched_slant_stack(self, n, n_batches, shift_bin, shift_frac, gain, windows, first, last, weights, p0=0.0, dp=0.0,
                                smooth=0, amplitude=1, first_id=0, seed=0x5EED):
        """run_batched that also makes the slant stack of the receivers first .. last where the batch blocks lie (include/r3d.h
        r3d_run_batched_slant_stack): shift_bin, shift_frac [M, A] (slant_shifts makes them), gain [A] and windows [W, 2] on
        the host.  Returns (Result, energy_se, counts_se, slant): a dict of stack, stack_se [M, n_bins], fold [M, n_bins]
        (uint32), power, power_se [W, M], picks, picks_se [W, 4]."""
        m = self.model
        A = int(last) - int(first) + 1
        if A < 1:
            raise ValueError("the array needs first <= last")
        k = np.ascontiguousarray(shift_bin, dtype=np.int32)
        f = np.ascontiguousarray(shift_frac, dtype=np.float64)
        g = np.ascontiguousarray(gain, dtype=np.float64)
        w = np.ascontiguousarray(windows, dtype=np.uint32).reshape(-1, 2)
        M, W = k.shape[0], w.shape[0]
        if k.shape != (M, A) or f.shape != (M, A) or g.shape != (A,):
            raise ValueError("shift_bin and shift_frac must be [M, A] and gain [A]")
        spec = slant_spec(m.n_seismometers, m.n_bins, first, last, weights, k.ctypes.data, f.ctypes.data, g.ctypes.data,
                          w.ctypes.data if W else None, M, W, p0, dp, smooth, amplitude)
        got = dict(stack=np.zeros((M, m.n_bins)), stack_se=np.zeros((M, m.n_bins)), fold=np.zeros((M, m.n_bins), dtype=np.uint32),
                   power=np.zeros((W, M)), power_se=np.zeros((W, M)), picks=np.zeros((W, _ffi.R3D_SLANT_N)),
                   picks_se=np.zeros((W, _ffi.R3D_SLANT_N)))
        out = _ffi.SlantResult(size=C.sizeof(_ffi.SlantResult), **{name: v.ctypes.data for name, v in got.items()})
        res, ese, cse = _run_batched_to_host(self._lib, "r3d_run_batched_slant_stack", self._e, m, n, first_id, seed, n_batches,
                                             None, C.byref(spec), C.byref(out))
        return res, ese, cse, got

    def run_batched_contrast(self, other, n, n_other, n_batches, other_batches, first, last, weights, bins=None, regions=(), gain=None,
                             scale=None, smooth=0, first_id=0, seed=0x5EED, other_seed=0x5EED + 1):
        """run_batched of this engine (the BASE: n histories in n_batches batches under `seed`) and then of `other` (the TEST:
        n_other, other_batches, other_seed), with the contrast of the receivers first .. last made where both runs' batch
        blocks lie (include/r3d.h r3d_run_batched_contrast): bins [A, W, 2] and gain [A] on the host, regions (i0, i1) pairs of
        array indices, scale the two sides' multipliers (None: (1, n / n_other)).  Returns ((Result, energy_se, counts_se) of
        the base, the same of the test, contrast): a dict of contrast, contrast_se [A, n_bins], lit [A] (uint32), window,
        window_se [A, W, 3], region, region_se [R, W, 3], region_loo [R, W, n_batches + other_batches]."""
        m, mo = self.model, other.model
        for what in ("n_seismometers", "n_bins"):
            if getattr(m, what) != getattr(mo, what):
                raise ValueError(f"the two models' {what} differ")
        if m.desc.params.time_per_bin != mo.desc.params.time_per_bin:
            raise ValueError("the two models' time_per_bin differ")
        A = int(last) - int(first) + 1
        if A < 1:
            raise ValueError("the array needs first <= last")
        b = np.ascontiguousarray(bins, dtype=np.uint32) if bins is not None else np.zeros((A, 0, 2), dtype=np.uint32)
        if b.ndim != 3 or b.shape[0] != A or b.shape[2] != 2:
            raise ValueError("bins must be [A, W, 2]")
        W, R = b.shape[1], len(regions)
        g = np.ascontiguousarray(gain, dtype=np.float64) if gain is not None else None
        if g is not None and g.shape != (A,):
            raise ValueError("gain must be [A]")
        Ba, Bb = max(int(n_batches), 0), max(int(other_batches), 0)
        spec = contrast_spec(m.n_seismometers, m.n_bins, first, last, weights, b.ctypes.data if W else None,
                             g.ctypes.data if g is not None else None, W, regions,
                             scale if scale is not None else (1.0, float(n) / float(n_other) if n_other else 1.0), smooth)
        N3 = _ffi.R3D_CONTRAST_N
        got = dict(contrast=np.zeros((A, m.n_bins)), contrast_se=np.zeros((A, m.n_bins)), lit=np.zeros(A, dtype=np.uint32),
                   window=np.zeros((A, W, N3)), window_se=np.zeros((A, W, N3)), region=np.zeros((R, W, N3)),
                   region_se=np.zeros((R, W, N3)), region_loo=np.zeros((R, W, Ba + Bb)))
        out = _ffi.ContrastResult(size=C.sizeof(_ffi.ContrastResult), **{name: v.ctypes.data for name, v in got.items()})
        shape = (m.n_seismometers, m.n_bins)
        sides = []
        for model in (m, mo):
            res = model.new_result()
            sides.append([res, res._as_c(), np.zeros(shape + (_ffi.R3D_N_ENERGY,)), np.zeros(shape + (_ffi.R3D_N_COUNT,))])
        (ra, ca, esa, csa), (rb, cb, esb, csb) = sides
        if self._lib.r3d_run_batched_contrast(self._e, other._e, n, n_other, first_id, seed, other_seed, n_batches, other_batches,
                                              C.byref(ca), C.byref(cb), esa.ctypes.data_as(_ffi._dp), csa.ctypes.data_as(_ffi._dp),
                                              esb.ctypes.data_as(_ffi._dp), csb.ctypes.data_as(_ffi._dp), C.byref(spec), C.byref(out)):
            raise RuntimeError("r3d_run_batched_contrast failed: " + self._lib.r3d_last_error().decode())
        ra._from_c(ca)
        rb._from_c(cb)
        return (ra, esa, csa), (rb, esb, csb), got

    def run_device(self, n, first_id, seed, d_energy, d_counts, d_scalars, stream=None, carry=None):
        """Asynchronous, device-resident accumulate (pointers are raw device
        addresses, e.g. tensor.data_ptr()).  carry: None (a self-contained launch),
        "carry" (one of a chain: unfinished histories stay in the engine for its next
        launch) or "final" (resume and finish everything carried); see r3d_run_device_carry."""
        if carry not in (None, "carry", "final"):
            raise ValueError(f"carry must be None, 'carry' or 'final', not {carry!r}")
        if carry is not None:
            rc = self._lib.r3d_run_device_carry(self._e, n, first_id, seed, d_energy, d_counts, d_scalars,
                                                stream, 1 if carry == "final" else 0)
        else:
            rc = self._lib.r3d_run_device(self._e, n, first_id, seed, d_energy, d_counts, d_scalars,
                                          None, stream)
        if rc:
            raise RuntimeError("r3d_run_device failed: " + self._lib.r3d_last_error().decode())

    # -- volumetric scatter-event grid (config 5 of BASELINE.json) -----------
    def set_volume(self, origin, cell_size, dims, n_frames, frame_dt):
        """Attach count[type][frame][z][y][x] (uint32, HBM) filled at SCT / REF events."""
        v = volume_desc(origin, cell_size, dims, n_frames, frame_dt)
        if self._lib.r3d_engine_set_volume(self._e, C.byref(v)):
            raise RuntimeError("r3d_engine_set_volume failed: " + self._lib.r3d_last_error().decode())
        self._vol_shape = (2, int(n_frames), int(dims[2]), int(dims[1]), int(dims[0]))

    def set_volume_buffer(self, origin, cell_size, dims, n_frames, frame_dt, counters):
        """The same grid in caller-owned device memory: `counters` is a contiguous 32-bit integer
        tensor of 2*n_frames*nz*ny*nx zeroed elements (e.g. a torch tensor that is reduced over
        ranks afterwards).  The engine writes through its raw address, so this object keeps a
        reference to the tensor until the grid is detached or the engine closed."""
        shape = (2, int(n_frames), int(dims[2]), int(dims[1]), int(dims[0]))
        want = 1
        for d in shape:
            want *= d
        if not hasattr(counters, "data_ptr"):
            raise TypeError("set_volume_buffer takes the tensor itself, not an address: the engine "
                            "must keep it alive while it adds into it")
        if counters.numel() != want or counters.element_size() != 4 or not counters.is_contiguous():
            raise ValueError(f"volume buffer must be {want} contiguous 32-bit counters, got "
                             f"{counters.numel()} x {counters.element_size()} bytes")
        v = volume_desc(origin, cell_size, dims, n_frames, frame_dt)
        if self._lib.r3d_engine_set_volume_buffer(self._e, C.byref(v), counters.data_ptr()):
            raise RuntimeError("r3d_engine_set_volume_buffer failed: " + self._lib.r3d_last_error().decode())
        assert self._lib.r3d_volume_len(self._e) == want
        self._volume_keepalive = counters
        self._vol_shape = shape

    def detach_volume(self):
        """Stop binning events (r3d_engine_set_volume_buffer(NULL)); releases the caller's tensor."""
        if getattr(self, "_e", None):
            if self._lib.r3d_engine_set_volume_buffer(self._e, None, None):
                raise RuntimeError("detaching the volume failed: " + self._lib.r3d_last_error().decode())
        self._volume_keepalive = None

    def set_production_finals(self, base_id, capacity):
        """Final records out of the production kernels for ids [base_id, base_id + capacity) (capacity 0: off)."""
        if self._lib.r3d_engine_set_production_finals(self._e, base_id, capacity):
            raise RuntimeError("r3d_engine_set_production_finals failed: " + self._lib.r3d_last_error().decode())

    def production_finals(self, first, count):
        out = (_ffi.Final * count)()
        if self._lib.r3d_production_finals_read(self._e, out, first, count):
            raise RuntimeError("r3d_production_finals_read failed: " + self._lib.r3d_last_error().decode())
        return out

    def read_volume(self, reset=False):
        out = np.zeros(self._vol_shape, dtype=np.uint32)
        assert out.size == self._lib.r3d_volume_len(self._e)
        if self._lib.r3d_volume_read(self._e, out.ctypes.data_as(C.POINTER(C.c_uint32)), int(reset)):
            raise RuntimeError("r3d_volume_read failed: " + self._lib.r3d_last_error().decode())
        return out

    def volume_device_ptr(self):
        return self._lib.r3d_volume_device_ptr(self._e)

    # -- scattering tables as the engine holds them ------------------------------
    def scatterer_stats(self, s):
        """[mfp_p, mfp_s, dipole_p, dipole_s, total_pp, total_ps, total_sp, total_ss]"""
        out = (C.c_double * 8)()
        if self._lib.r3d_engine_scatterer_stats(self._e, s, out):
            raise IndexError(s)
        return list(out)

    def download_scatterer(self, s):
        """(cdf[4, n_toa], spol[n_toa]) copied from HBM."""
        n = self.model.n_toa
        cdf, spol = np.zeros((4, n)), np.zeros(n)
        ptrs = (_ffi._dp * 4)(*[cdf[k].ctypes.data_as(_ffi._dp) for k in range(4)])
        if self._lib.r3d_engine_download_scatterer(self._e, s, ptrs, spol.ctypes.data_as(_ffi._dp)):
            raise RuntimeError("download failed: " + self._lib.r3d_last_error().decode())
        return cdf, spol

    def download_source(self):
        """(cdf[3, n_toa], whole[3]): the source's cumulative P / SH / SV tables as the engine holds them."""
        n = self.model.n_toa
        cdf, whole = np.zeros((3, n)), np.zeros(3)
        ptrs = (_ffi._dp * 3)(*[cdf[k].ctypes.data_as(_ffi._dp) for k in range(3)])
        if self._lib.r3d_engine_download_source(self._e, ptrs, whole.ctypes.data_as(_ffi._dp)):
            raise RuntimeError("download failed: " + self._lib.r3d_last_error().decode())
        return cdf, whole

    def download_toa(self):
        """toa[n_toa, 2]: the take-off set (theta, phi) as the engine holds it."""
        toa = np.zeros((self.model.n_toa, 2))
        if self._lib.r3d_engine_download_toa(self._e, toa.ctypes.data_as(_ffi._dp)):
            raise RuntimeError("download failed: " + self._lib.r3d_last_error().decode())
        return toa

    # -- per-event report stream (the reference's --reports) -------------------
    def set_event_log(self, mask=_ffi.R3D_RPT_ALL, capacity=1 << 20):
        """Attach an HBM buffer of `capacity` r3d_event records for the tags in `mask`."""
        if self._lib.r3d_engine_set_event_log(self._e, int(mask), int(capacity)):
            raise RuntimeError("r3d_engine_set_event_log failed: " + self._lib.r3d_last_error().decode())
        self._ev_cap = int(capacity) if mask else 0

    def event_log_count(self):
        return int(self._lib.r3d_event_log_count(self._e))

    def read_event_log(self, reset=False):
        """Stored records as a numpy structured array (_ffi.event_dtype)."""
        n = min(self.event_log_count(), self._ev_cap)
        out = np.zeros(n, dtype=_ffi.event_dtype())
        got = self._lib.r3d_event_log_read(self._e, out.ctypes.data, n, int(reset))
        if got == (1 << 64) - 1:
            raise RuntimeError("r3d_event_log_read failed: " + self._lib.r3d_last_error().decode())
        return out[:got]

    @property
    def variant(self):
        """(cell kind, table residency) of the compiled kernel this engine launches:
        kind 0 cylinder / 1 tetra / 2 sphere shell; residency 0 cells + scatterer heads in LDS,
        1 heads only, 2 neither."""
        v = int(self._lib.r3d_engine_variant(self._e))
        return v // 4, v % 4

    @property
    def pool_slots(self):
        return int(self._lib.r3d_engine_pool_slots(self._e))

    @property
    def accumulators(self):
        """entries of a workgroup's LDS table of bin accumulators"""
        return int(self._lib.r3d_engine_accumulators(self._e))

    def last_kernel_ms(self):
        return float(self._lib.r3d_last_kernel_ms(self._e))

    def launch_count(self):
        """Launches enqueued so far; launch ids run from 1."""
        return int(self._lib.r3d_launch_count(self._e))

    def kernel_ms(self, launch):
        """Kernel time of launch id `launch` (one of the 64 most recent), -1 if not on record."""
        return float(self._lib.r3d_kernel_ms(self._e, int(launch)))
