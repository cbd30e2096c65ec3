"""radiative3d_amd -- MI355X-native engine for the Phonon::Propagate hot path
of Radiative3D.  Host model builder in C++ (host/), HIP
kernels + C-ABI in csrc/, batch statistics on top of it in stats/, the array image in arrays/, the envelope shape in shapes/, the envelope misfit in fits/, the slant stack in beams/, the contrast of two runs in contrasts/, thin ctypes mirror here."""
from .model import Engine, Model, Node, Result, array_contrast, array_image, array_powerlaw, batch_merge, batch_moments, batch_partial, contrast_decibel, contrast_gains, envelope_misfit, envelope_shape, precision_judge, project_volume, range_bins, run_model, slant_shifts, slant_stack, time_maps_volume, window_bins, window_log_ratio, window_sums  # noqa: F401

__all__ = ["Model", "Engine", "Node", "Result", "run_model", "batch_moments", "batch_partial", "batch_merge", "precision_judge", "range_bins", "project_volume", "time_maps_volume", "window_sums", "window_bins", "window_log_ratio", "array_image", "array_powerlaw", "envelope_shape", "envelope_misfit", "slant_shifts", "slant_stack", "array_contrast", "contrast_gains", "contrast_decibel"]
