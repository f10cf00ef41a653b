"""recfilter_amd -- MI355X-native tiled recursive (IIR) filters.

The product is recfilter_amd/librecfilter_amd.so (hand-written gfx950 HIP kernels behind the
C ABI of include/recfilter_amd.h).  This package is the host-side mirror of the reference's
RecFilter front-end plus the ctypes plumbing to reach the library; it contains no fallback
implementation of the filter.
"""
from . import capi
from .capi import RecFilterError, build_library
from .filter import (Pointwise, RecFilter, RecFilterDim, RecFilterDimAndCausality, RecFilterSchedule,
                     RecFilterUsageError)
from .plan import (Plan, box_difference, tap_filter, stream_copy_ms, gaussian_box_filter, second_order_sections, gaussian_weights, integral_image_coeff,
                   overlap_feedback_coeff, recursive_filter)
from .varscan import (SmoothPlan, VarPlan, domain_transform_bases, domain_transform_distances, domain_transform_distances_backward,
                      domain_transform_distances_volume, domain_transform_distances_volume_backward, domain_transform_weights, edge_aware_smooth, edge_aware_smooth_volume, smooth_samples,
                      var_scan, var_scan_signal, var_scan_volume)
from .var2 import (BiquadCascadeStream, Var2Plan, allpole_scan, biquad_cascade, biquad_cascade_frames, biquad_cascade_frames_stream, biquad_scan,
                   biquad_scan_frames, expand_frames, frames_count)

__all__ = [
    "capi", "RecFilterError", "build_library", "Pointwise", "RecFilter", "RecFilterDim", "RecFilterDimAndCausality",
    "RecFilterSchedule", "RecFilterUsageError", "Plan", "box_difference", "tap_filter", "second_order_sections", "gaussian_box_filter", "gaussian_weights",
    "integral_image_coeff", "overlap_feedback_coeff", "VarPlan", "domain_transform_weights", "edge_aware_smooth",
    "domain_transform_bases", "domain_transform_distances", "SmoothPlan", "var_scan", "var_scan_signal", "smooth_samples",
    "domain_transform_distances_backward", "recursive_filter", "var_scan_volume", "domain_transform_distances_volume",
    "edge_aware_smooth_volume", "domain_transform_distances_volume_backward",
    "Var2Plan", "allpole_scan", "biquad_scan", "biquad_cascade", "biquad_cascade_frames", "biquad_cascade_frames_stream", "BiquadCascadeStream", "biquad_scan_frames", "expand_frames", "frames_count",
]
