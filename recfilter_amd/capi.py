"""ctypes binding of the C ABI declared in include/recfilter_amd.h.

This is plumbing: every call goes straight into librecfilter_amd.so (hand-written gfx950
kernels).  There is no Python or CPU implementation of the filter behind it -- if the shared
library is missing, importing this module raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
# RECFILTER_AMD_LIB: load another build of the same library (A/B timing of kernel changes)
LIB_PATH = os.environ.get("RECFILTER_AMD_LIB") or os.path.join(_PKG, "librecfilter_amd.so")
CSRC = os.path.join(_PKG, "csrc")

RF_MAX_DIMS = 3
RF_MAX_ORDER = 32
RF_ABI = 3          # revision of include/recfilter_amd.h this module mirrors (rf_filter_desc.abi)
RF_MAX_SCANS = 32
RF_MAX_PLANES = 16
RF_VAR_MAX_SCANS = 8     # scans (and weight planes) of a plan of spatially varying scans (rf_var_desc)
RF_SMOOTH_MAX_ITERATIONS = 8     # iterations of a smoothing plan (rf_smooth_desc)
RF_SMOOTH_MAX_BATCH = 1024       # images of a batched smoothing plan (rf_smooth_batch_desc)
RF_DEVICE_HOST_ONLY = -2
RF_SMOOTH_VOLUME_BACKWARD = 1    # rf_smooth_volume_desc.flags: the volume plan has a backward (f32 volumes)

RF_OK, RF_ERR_INVALID_ARG, RF_ERR_UNSUPPORTED, RF_ERR_HIP, RF_ERR_NOMEM, RF_ERR_STATE = range(6)
RF_F32, RF_F64, RF_I32, RF_I16, RF_F16, RF_BF16 = range(6)      # RF_F16 / RF_BF16: 16-bit float STORAGE, f32 arithmetic
RF_BORDER_ZERO, RF_BORDER_CLAMP = 0, 1
RF_POINTWISE_PRE, RF_POINTWISE_POST = 1, 2
RF_IN_PIXEL, RF_IN_U8, RF_IO_U8 = 0, 1, 2      # rf_input_dtype; RF_IO_U8: byte planes on both sides, out = sat8(f32 result)
RF_BUFFER_TABLE, RF_BUFFER_ZEROED, RF_BUFFER_SCRATCH = range(3)      # rf_buffer_kind (rf_plan_debug_buffer_kind)
BUFFER_KIND_NAMES = {RF_BUFFER_TABLE: "table", RF_BUFFER_ZEROED: "zeroed", RF_BUFFER_SCRATCH: "scratch"}
RF_PATH_AUTO, RF_PATH_UNTILED, RF_PATH_TILED_GENERIC, RF_PATH_TILED_FUSED, RF_PATH_TILED_OVERLAPPED, RF_PATH_TILED_MATRIX = range(6)
# rf_filter_desc.flags (plan options; the library reads no environment variable)
RF_PLAN_FORCE_EXCHANGE, RF_PLAN_TILED_ONLY, RF_PLAN_NO_CASCADE, RF_PLAN_NO_SECTIONS = 0x01, 0x02, 0x04, 0x08
RF_PLAN_NO_PLANE_BATCH, RF_PLAN_STREAM_PASS1, RF_PLAN_STAGED_PASS1, RF_PLAN_LATE_EXCHANGE = 0x10, 0x20, 0x40, 0x80
RF_PLAN_SERIAL_UNTILED = 0x01000000
RF_PLAN_MFMA_PASS1 = 0x02000000
RF_PLAN_WALK_PASS1 = 0x04000000
RF_PLAN_NO_OVERLAP = 0x08000000
RF_PLAN_INPLACE_Z = 0x10000000
RF_PLAN_FULL_CARRY_SCAN = 0x20000000
RF_PLAN_STAGE_HALF = 0x40000000       # 16-bit float pixels: staged through f32 planes even where the fused kernels run them
RF_PLAN_SEPARATE_ROW_SCANS = 0x80000000       # a neighbour-form step keeps its three kernels (rf_plan_table("row_scans") = 0)


def RF_PLAN_TILE_ROWS(n: int) -> int:
    return (int(n) & 0xff) << 8


def RF_PLAN_TILE_PLANES(n: int) -> int:
    return (int(n) & 0xff) << 16


PATH_NAMES = {RF_PATH_AUTO: "auto", RF_PATH_UNTILED: "untiled",
              RF_PATH_TILED_GENERIC: "tiled_generic", RF_PATH_TILED_FUSED: "tiled_fused",
              RF_PATH_TILED_OVERLAPPED: "tiled_overlapped", RF_PATH_TILED_MATRIX: "tiled_matrix"}

# every symbol include/recfilter_amd.h declares
EXPORTED_SYMBOLS = [
    "rf_plan_create", "rf_plan_destroy", "rf_plan_workspace_bytes", "rf_plan_num_instances", "rf_plan_path", "rf_plan_tiles",
    "rf_plan_num_kernels", "rf_plan_execute", "rf_plan_execute_timed", "rf_plan_num_exchanges",
    "rf_plan_exchange_bytes",
    "rf_plan_begin", "rf_plan_exchange_local", "rf_plan_exchange_apply", "rf_plan_has_interior", "rf_plan_interior", "rf_plan_finish", "rf_plan_abort",
    "rf_plan_table", "rf_plan_debug_buffer", "rf_plan_debug_buffer_kind", "rf_plan_debug_fill", "rf_gaussian_weights", "rf_integral_image_coeff", "rf_overlap_feedback_coeff",
    "rf_gaussian_box_filter", "rf_box_difference", "rf_tap_filter", "rf_stream_copy", "rf_last_error_string", "rf_version", "rf_device_count",
    "rf_var_plan_create", "rf_var_plan_destroy", "rf_var_plan_workspace_bytes", "rf_var_plan_num_kernels", "rf_var_plan_execute",
    "rf_var_plan_execute_timed", "rf_var_plan_execute_power", "rf_var_plan_execute_power_timed", "rf_var_distances",
    "rf_var_plan_backward", "rf_var_plan_backward_timed", "rf_var_plan_backward_num_kernels", "rf_var_plan_backward_workspace_bytes",
    "rf_smooth_plan_create", "rf_smooth_plan_destroy", "rf_smooth_plan_workspace_bytes", "rf_smooth_plan_num_kernels",
    "rf_smooth_plan_bases", "rf_smooth_plan_execute", "rf_smooth_plan_execute_timed",
    "rf_var_plan_backward_power", "rf_var_plan_backward_power_timed", "rf_var_distances_backward",
    "rf_smooth_plan_backward", "rf_smooth_plan_backward_timed", "rf_smooth_plan_backward_num_kernels",
    "rf_smooth_plan_backward_workspace_bytes", "rf_smooth_plan_create_batched",
    "rf_plan_backward", "rf_plan_backward_timed", "rf_plan_backward_num_kernels", "rf_plan_backward_workspace_bytes",
    "rf_var_plan_create_signal",
    "rf_var_plan_create_volume", "rf_var_distances_volume", "rf_smooth_plan_create_volume",
    "rf_var_distances_volume_backward",
    "rf_var_plan_backward_power_bases", "rf_var_plan_backward_power_bases_timed", "rf_var_plan_backward_bases_num_kernels",
    "rf_var_plan_backward_bases_workspace_bytes", "rf_smooth_plan_set_sigmas",
    "rf_smooth_plan_backward_sigmas", "rf_smooth_plan_backward_sigmas_timed", "rf_smooth_plan_backward_sigmas_num_kernels",
    "rf_var2_plan_create_signal", "rf_var2_plan_destroy", "rf_var2_plan_workspace_bytes", "rf_var2_plan_num_kernels",
    "rf_var2_plan_execute", "rf_var2_plan_execute_timed", "rf_var2_plan_backward", "rf_var2_plan_backward_timed",
    "rf_var2_plan_backward_num_kernels",
    "rf_var2_plan_execute_biquad", "rf_var2_plan_execute_biquad_timed", "rf_var2_plan_backward_biquad", "rf_var2_plan_backward_biquad_timed",
    "rf_var2_plan_biquad_num_kernels", "rf_var2_plan_backward_biquad_num_kernels", "rf_var2_plan_backward_biquad_bytes",
    "rf_var2_plan_execute_cascade", "rf_var2_plan_execute_cascade_timed", "rf_var2_plan_backward_cascade",
    "rf_var2_plan_backward_cascade_timed", "rf_var2_plan_cascade_num_kernels", "rf_var2_plan_backward_cascade_num_kernels",
    "rf_var2_plan_backward_cascade_bytes",
    "rf_var2_plan_execute_cascade_keep", "rf_var2_plan_execute_cascade_keep_timed", "rf_var2_plan_backward_cascade_kept",
    "rf_var2_plan_backward_cascade_kept_timed", "rf_var2_plan_backward_cascade_kept_num_kernels",
    "rf_var2_plan_backward_cascade_kept_bytes",
    "rf_var2_frames_count", "rf_var2_expand_frames", "rf_var2_plan_execute_biquad_frames", "rf_var2_plan_execute_biquad_frames_timed",
    "rf_var2_plan_backward_biquad_frames", "rf_var2_plan_backward_biquad_frames_timed", "rf_var2_plan_biquad_frames_num_kernels",
    "rf_var2_plan_backward_biquad_frames_num_kernels", "rf_var2_plan_backward_biquad_frames_bytes",
    "rf_var2_plan_execute_cascade_frames", "rf_var2_plan_execute_cascade_frames_timed", "rf_var2_plan_backward_cascade_frames",
    "rf_var2_plan_backward_cascade_frames_timed", "rf_var2_plan_cascade_frames_num_kernels",
    "rf_var2_plan_backward_cascade_frames_num_kernels", "rf_var2_plan_backward_cascade_frames_bytes",
    "rf_var2_plan_execute_cascade_frames_stream", "rf_var2_plan_execute_cascade_frames_stream_timed",
    "rf_var2_plan_cascade_frames_stream_num_kernels", "rf_var2_plan_cascade_frames_stream_state_bytes",
    "rf_var2_plan_backward_cascade_frames_stream", "rf_var2_plan_backward_cascade_frames_stream_timed",
    "rf_var2_plan_backward_cascade_frames_stream_num_kernels",
]


class ScanDesc(ctypes.Structure):
    _fields_ = [("dim", ctypes.c_int32), ("causal", ctypes.c_int32), ("order", ctypes.c_int32),
                ("feedfwd", ctypes.c_float), ("feedback", ctypes.c_float * RF_MAX_ORDER)]


class PointwiseDesc(ctypes.Structure):
    _fields_ = [("flags", ctypes.c_int32), ("pre_scale", ctypes.c_float), ("pre_bias", ctypes.c_float),
                ("post_filtered", ctypes.c_float), ("post_input", ctypes.c_float), ("post_bias", ctypes.c_float),
                ("in_dtype", ctypes.c_int32)]


class FilterDesc(ctypes.Structure):
    _fields_ = [("ndim", ctypes.c_int32), ("abi", ctypes.c_uint32), ("extent", ctypes.c_int64 * RF_MAX_DIMS),
                ("dtype", ctypes.c_int32), ("n_planes", ctypes.c_int32), ("border", ctypes.c_int32),
                ("n_scans", ctypes.c_int32), ("scans", ctypes.POINTER(ScanDesc)),
                ("tile", ctypes.c_int32 * RF_MAX_DIMS), ("path", ctypes.c_int32),
                ("device", ctypes.c_int32), ("shard_rank", ctypes.c_int32), ("shard_world", ctypes.c_int32),
                ("pointwise", PointwiseDesc), ("shard_extents", ctypes.POINTER(ctypes.c_int64)),
                ("flags", ctypes.c_uint32)]


class Tap(ctypes.Structure):
    _fields_ = [("plane", ctypes.c_int32), ("offset", ctypes.c_int32 * RF_MAX_DIMS), ("weight", ctypes.c_float)]


class VarScanDesc(ctypes.Structure):
    _fields_ = [("dim", ctypes.c_int32), ("causal", ctypes.c_int32), ("weights", ctypes.c_int32)]


class VarDesc(ctypes.Structure):
    _fields_ = [("ndim", ctypes.c_int32), ("abi", ctypes.c_uint32), ("extent", ctypes.c_int64 * RF_MAX_DIMS),
                ("dtype", ctypes.c_int32), ("n_planes", ctypes.c_int32), ("n_weights", ctypes.c_int32),
                ("n_scans", ctypes.c_int32), ("scans", ctypes.POINTER(VarScanDesc)),
                ("device", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class VarSignalDesc(ctypes.Structure):
    _fields_ = [("abi", ctypes.c_uint32), ("length", ctypes.c_int64), ("dtype", ctypes.c_int32), ("n_planes", ctypes.c_int32),
                ("n_weights", ctypes.c_int32), ("n_scans", ctypes.c_int32), ("scans", ctypes.POINTER(VarScanDesc)),
                ("device", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class VarVolumeDesc(ctypes.Structure):
    _fields_ = [("abi", ctypes.c_uint32), ("width", ctypes.c_int64), ("height", ctypes.c_int64), ("depth", ctypes.c_int64),
                ("dtype", ctypes.c_int32), ("n_planes", ctypes.c_int32), ("n_weights", ctypes.c_int32), ("n_scans", ctypes.c_int32),
                ("scans", ctypes.POINTER(VarScanDesc)), ("device", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class Var2SignalDesc(ctypes.Structure):
    _fields_ = [("abi", ctypes.c_uint32), ("length", ctypes.c_int64), ("n_lines", ctypes.c_int32), ("stride", ctypes.c_int64),
                ("causal", ctypes.c_int32), ("device", ctypes.c_int32), ("flags", ctypes.c_uint32)]


RF_VAR2_MAX_SECTIONS = 16


class Var2Section(ctypes.Structure):
    """rf_var2_section, and rf_var2_section_grad: five addresses"""
    _fields_ = [("b0", ctypes.c_void_p), ("b1", ctypes.c_void_p), ("b2", ctypes.c_void_p), ("a1", ctypes.c_void_p), ("a2", ctypes.c_void_p)]


class SmoothDesc(ctypes.Structure):
    _fields_ = [("abi", ctypes.c_uint32), ("image_u8", ctypes.c_int32), ("width", ctypes.c_int64), ("height", ctypes.c_int64),
                ("n_planes", ctypes.c_int32), ("n_guide", ctypes.c_int32), ("guide_u8", ctypes.c_int32),
                ("iterations", ctypes.c_int32), ("sigma_s", ctypes.c_double), ("sigma_r", ctypes.c_double),
                ("device", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class SmoothVolumeDesc(ctypes.Structure):
    _fields_ = [("abi", ctypes.c_uint32), ("image_u8", ctypes.c_int32), ("width", ctypes.c_int64), ("height", ctypes.c_int64),
                ("depth", ctypes.c_int64), ("n_planes", ctypes.c_int32), ("n_guide", ctypes.c_int32), ("guide_u8", ctypes.c_int32),
                ("iterations", ctypes.c_int32), ("sigma_s", ctypes.c_double), ("sigma_r", ctypes.c_double),
                ("spacing_z", ctypes.c_double), ("device", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class SmoothBatchDesc(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("image_stride", ctypes.c_int64), ("guide_stride", ctypes.c_int64)]


class RecFilterError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"recfilter_amd status {status}: {message}")
        self.status = status


def build_library(force: bool = False) -> str:
    """Compile every HIP source for gfx950 into recfilter_amd/librecfilter_amd.so (in-tree)."""
    cmd = ["make", "-C", CSRC, "-j4"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib() -> ctypes.CDLL:
    """Load librecfilter_amd.so.  torch is imported first so that both share ONE HIP runtime
    (torch bundles its own libamdhip64 with the same SONAME as /opt/rocm's)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C {CSRC}` (or __graft_entry__.build()); "
            "recfilter_amd has no fallback implementation")
    try:
        import torch  # noqa: F401  (loads torch's libamdhip64 before ours resolves the SONAME)
    except Exception:  # pragma: no cover - torch is plumbing, the library works without it
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, vpp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)
    fp = ctypes.POINTER(ctypes.c_float)
    L.rf_plan_create.argtypes = [ctypes.POINTER(FilterDesc), vpp]
    L.rf_plan_destroy.argtypes = [vp]
    L.rf_plan_workspace_bytes.argtypes = [vp]
    L.rf_plan_workspace_bytes.restype = ctypes.c_size_t
    L.rf_plan_num_instances.argtypes = [vp]
    L.rf_plan_path.argtypes = [vp]
    L.rf_plan_tiles.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.rf_plan_num_kernels.argtypes = [vp]
    L.rf_plan_execute.argtypes = [vp, vpp, vpp, vp]
    L.rf_plan_execute_timed.argtypes = [vp, vpp, vpp, vp, fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_plan_num_exchanges.argtypes = [vp]
    L.rf_plan_begin.argtypes = [vp, vpp, vpp, vp]
    L.rf_plan_exchange_bytes.argtypes = [vp, ctypes.c_int]
    L.rf_plan_exchange_bytes.restype = ctypes.c_size_t
    L.rf_plan_exchange_local.argtypes = [vp, ctypes.c_int, vp]
    L.rf_plan_exchange_apply.argtypes = [vp, ctypes.c_int, vp]
    L.rf_plan_finish.argtypes = [vp]
    L.rf_plan_abort.argtypes = [vp]
    L.rf_plan_has_interior.argtypes = [vp]
    L.rf_plan_interior.argtypes = [vp]
    L.rf_plan_table.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.c_size_t,
                                ctypes.POINTER(ctypes.c_size_t)]
    L.rf_plan_debug_buffer.argtypes = [vp, ctypes.c_int, vpp, ctypes.POINTER(ctypes.c_size_t)]
    L.rf_plan_debug_buffer_kind.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.rf_plan_debug_fill.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
    L.rf_plan_backward.argtypes = [vp, vpp, vpp, vpp, vp, vp]
    L.rf_plan_backward_timed.argtypes = [vp, vpp, vpp, vpp, vp, vp, fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_plan_backward_num_kernels.argtypes = [vp, ctypes.c_int]
    L.rf_plan_backward_workspace_bytes.argtypes = [vp, ctypes.c_int]
    L.rf_plan_backward_workspace_bytes.restype = ctypes.c_size_t
    L.rf_gaussian_weights.argtypes = [ctypes.c_float, ctypes.c_int, fp]
    L.rf_integral_image_coeff.argtypes = [ctypes.c_int, fp]
    L.rf_overlap_feedback_coeff.argtypes = [fp, ctypes.c_int, fp, ctypes.c_int, fp]
    L.rf_gaussian_box_filter.argtypes = [ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_int)]
    L.rf_box_difference.argtypes = [vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_int32), vp]
    L.rf_stream_copy.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int64, vp]
    L.rf_tap_filter.argtypes = [vpp, ctypes.c_int, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int,
                                ctypes.POINTER(Tap), ctypes.c_int, vp]
    L.rf_var_plan_create.argtypes = [ctypes.POINTER(VarDesc), vpp]
    L.rf_var_plan_create_signal.argtypes = [ctypes.POINTER(VarSignalDesc), vpp]
    L.rf_var_plan_create_volume.argtypes = [ctypes.POINTER(VarVolumeDesc), vpp]
    L.rf_var_distances_volume.argtypes = [vpp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_float, ctypes.c_float, vp, vp, vp, ctypes.c_int32, vp]
    L.rf_smooth_plan_create_volume.argtypes = [ctypes.POINTER(SmoothVolumeDesc), vpp]
    L.rf_var_distances_volume_backward.argtypes = [vpp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_float,
                                                   vp, vp, vp, vpp, ctypes.c_int32, ctypes.c_int32, vp]
    L.rf_var_plan_destroy.argtypes = [vp]
    L.rf_var_plan_workspace_bytes.argtypes = [vp]
    L.rf_var_plan_workspace_bytes.restype = ctypes.c_size_t
    L.rf_var_plan_num_kernels.argtypes = [vp]
    L.rf_var_plan_execute.argtypes = [vp, vpp, vpp, vpp, vp]
    L.rf_var_plan_execute_timed.argtypes = [vp, vpp, vpp, vpp, vp, fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_var_plan_execute_power.argtypes = [vp, vpp, vpp, fp, vpp, vp]
    L.rf_var_plan_execute_power_timed.argtypes = [vp, vpp, vpp, fp, vpp, vp, fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_var_plan_backward.argtypes = [vp, vpp, vpp, vpp, vpp, vpp, vp]
    L.rf_var_plan_backward_timed.argtypes = [vp, vpp, vpp, vpp, vpp, vpp, vp, fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_var_plan_backward_num_kernels.argtypes = [vp, ctypes.c_int]
    L.rf_var_plan_backward_workspace_bytes.argtypes = [vp, ctypes.c_int]
    L.rf_var_plan_backward_workspace_bytes.restype = ctypes.c_size_t
    L.rf_var_distances.argtypes = [vpp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_float, vp, vp,
                                   ctypes.c_int32, vp]
    L.rf_smooth_plan_create.argtypes = [ctypes.POINTER(SmoothDesc), vpp]
    L.rf_smooth_plan_create_batched.argtypes = [ctypes.POINTER(SmoothDesc), ctypes.POINTER(SmoothBatchDesc), vpp]
    L.rf_smooth_plan_destroy.argtypes = [vp]
    L.rf_smooth_plan_workspace_bytes.argtypes = [vp]
    L.rf_smooth_plan_workspace_bytes.restype = ctypes.c_size_t
    L.rf_smooth_plan_num_kernels.argtypes = [vp]
    L.rf_smooth_plan_bases.argtypes = [vp, fp]
    L.rf_smooth_plan_set_sigmas.argtypes = [vp, ctypes.c_double, ctypes.c_double]
    L.rf_smooth_plan_execute.argtypes = [vp, vpp, vpp, vpp, vp]
    L.rf_smooth_plan_execute_timed.argtypes = [vp, vpp, vpp, vpp, vp, fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_var_plan_backward_power.argtypes = [vp, vpp, vpp, fp, vpp, vpp, vpp, vp]
    L.rf_var_plan_backward_power_timed.argtypes = [vp, vpp, vpp, fp, vpp, vpp, vpp, vp, fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_var_plan_backward_power_bases.argtypes = [vp, vpp, vpp, fp, vpp, vpp, vpp, vp, vp]
    L.rf_var_plan_backward_power_bases_timed.argtypes = [vp, vpp, vpp, fp, vpp, vpp, vpp, vp, vp, fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_var_plan_backward_bases_num_kernels.argtypes = [vp]
    L.rf_var_plan_backward_bases_workspace_bytes.argtypes = [vp]
    L.rf_var_plan_backward_bases_workspace_bytes.restype = ctypes.c_size_t
    L.rf_var_distances_backward.argtypes = [vpp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_float, vp, vp, vpp,
                                            ctypes.c_int32, ctypes.c_int32, vp]
    L.rf_smooth_plan_backward.argtypes = [vp, vpp, vpp, vpp, vpp, vpp, ctypes.c_int32, vp]
    L.rf_smooth_plan_backward_timed.argtypes = [vp, vpp, vpp, vpp, vpp, vpp, ctypes.c_int32, vp, fp, ctypes.POINTER(ctypes.c_char_p),
                                                ctypes.c_int]
    L.rf_smooth_plan_backward_num_kernels.argtypes = [vp, ctypes.c_int]
    L.rf_smooth_plan_backward_sigmas.argtypes = [vp, vpp, vpp, vpp, vpp, vpp, ctypes.c_int32, vp, vp]
    L.rf_smooth_plan_backward_sigmas_timed.argtypes = [vp, vpp, vpp, vpp, vpp, vpp, ctypes.c_int32, vp, vp, fp, ctypes.POINTER(ctypes.c_char_p),
                                                       ctypes.c_int]
    L.rf_smooth_plan_backward_sigmas_num_kernels.argtypes = [vp, ctypes.c_int]
    L.rf_smooth_plan_backward_workspace_bytes.argtypes = [vp, ctypes.c_int]
    L.rf_smooth_plan_backward_workspace_bytes.restype = ctypes.c_size_t
    L.rf_var2_plan_create_signal.argtypes = [ctypes.POINTER(Var2SignalDesc), vpp]
    L.rf_var2_plan_destroy.argtypes = [vp]
    L.rf_var2_plan_workspace_bytes.argtypes = [vp]
    L.rf_var2_plan_workspace_bytes.restype = ctypes.c_size_t
    L.rf_var2_plan_num_kernels.argtypes = [vp]
    L.rf_var2_plan_execute.argtypes = [vp, vp, vp, vp, vp, vp]
    L.rf_var2_plan_execute_timed.argtypes = [vp, vp, vp, vp, vp, vp, fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_var2_plan_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rf_var2_plan_backward_timed.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_var2_plan_backward_num_kernels.argtypes = [vp, ctypes.c_int]
    L.rf_var2_plan_execute_biquad.argtypes = [vp] * 9
    L.rf_var2_plan_execute_biquad_timed.argtypes = [vp] * 9 + [fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_var2_plan_backward_biquad.argtypes = [vp] * 16
    L.rf_var2_plan_backward_biquad_timed.argtypes = [vp] * 16 + [fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_var2_plan_biquad_num_kernels.argtypes = [vp]
    L.rf_var2_plan_backward_biquad_num_kernels.argtypes = [vp]
    L.rf_var2_plan_backward_biquad_bytes.argtypes = [vp]
    L.rf_var2_plan_backward_biquad_bytes.restype = ctypes.c_size_t
    sp, report = ctypes.POINTER(Var2Section), [fp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    L.rf_var2_plan_execute_cascade.argtypes = [vp, vp, sp, ctypes.c_int, vp, vp]
    L.rf_var2_plan_execute_cascade_timed.argtypes = [vp, vp, sp, ctypes.c_int, vp, vp] + report
    L.rf_var2_plan_backward_cascade.argtypes = [vp, vp, sp, ctypes.c_int, vp, vp, vp, sp, vp]
    L.rf_var2_plan_backward_cascade_timed.argtypes = [vp, vp, sp, ctypes.c_int, vp, vp, vp, sp, vp] + report
    L.rf_var2_plan_cascade_num_kernels.argtypes = [vp, ctypes.c_int]
    L.rf_var2_plan_backward_cascade_num_kernels.argtypes = [vp, ctypes.c_int]
    L.rf_var2_plan_backward_cascade_bytes.argtypes = [vp, ctypes.c_int]
    L.rf_var2_plan_backward_cascade_bytes.restype = ctypes.c_size_t
    kp = ctypes.POINTER(ctypes.c_void_p)      # the kept signals: an array of addresses
    L.rf_var2_plan_execute_cascade_keep.argtypes = [vp, vp, sp, ctypes.c_int, vp, kp, vp]
    L.rf_var2_plan_execute_cascade_keep_timed.argtypes = [vp, vp, sp, ctypes.c_int, vp, kp, vp] + report
    L.rf_var2_plan_backward_cascade_kept.argtypes = [vp, vp, sp, ctypes.c_int, kp, vp, vp, vp, sp, vp]
    L.rf_var2_plan_backward_cascade_kept_timed.argtypes = [vp, vp, sp, ctypes.c_int, kp, vp, vp, vp, sp, vp] + report
    L.rf_var2_plan_backward_cascade_kept_num_kernels.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.rf_var2_plan_backward_cascade_kept_bytes.argtypes = [vp, ctypes.c_int]
    L.rf_var2_plan_backward_cascade_kept_bytes.restype = ctypes.c_size_t
    L.rf_var2_frames_count.argtypes = [ctypes.c_int, ctypes.c_int]
    L.rf_var2_expand_frames.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64, vp, vp]
    frames = [vp, vp, sp, ctypes.c_int, ctypes.c_int, ctypes.c_int64]      # plan, in, the frames, hop, n_frames, frame_stride
    L.rf_var2_plan_execute_biquad_frames.argtypes = frames + [vp, vp]
    L.rf_var2_plan_execute_biquad_frames_timed.argtypes = frames + [vp, vp] + report
    L.rf_var2_plan_backward_biquad_frames.argtypes = frames + [vp, vp, vp, sp, vp]
    L.rf_var2_plan_backward_biquad_frames_timed.argtypes = frames + [vp, vp, vp, sp, vp] + report
    L.rf_var2_plan_biquad_frames_num_kernels.argtypes = [vp]
    L.rf_var2_plan_backward_biquad_frames_num_kernels.argtypes = [vp, ctypes.c_int]
    L.rf_var2_plan_backward_biquad_frames_bytes.argtypes = [vp, ctypes.c_int]
    L.rf_var2_plan_backward_biquad_frames_bytes.restype = ctypes.c_size_t
    # plan, in, the sections' frames, K, hop, n_frames, frame_stride
    cascade_frames = [vp, vp, sp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64]
    L.rf_var2_plan_execute_cascade_frames.argtypes = cascade_frames + [vp, kp, vp]
    L.rf_var2_plan_execute_cascade_frames_timed.argtypes = cascade_frames + [vp, kp, vp] + report
    L.rf_var2_plan_backward_cascade_frames.argtypes = cascade_frames + [kp, vp, vp, vp, sp, vp]
    L.rf_var2_plan_backward_cascade_frames_timed.argtypes = cascade_frames + [kp, vp, vp, vp, sp, vp] + report
    L.rf_var2_plan_cascade_frames_num_kernels.argtypes = [vp, ctypes.c_int]
    L.rf_var2_plan_backward_cascade_frames_num_kernels.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.rf_var2_plan_backward_cascade_frames_bytes.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.rf_var2_plan_backward_cascade_frames_bytes.restype = ctypes.c_size_t
    state = [vp, vp, ctypes.c_int64]      # state_in, state_out, state_stride
    L.rf_var2_plan_execute_cascade_frames_stream.argtypes = cascade_frames + [vp, kp] + state + [vp]
    L.rf_var2_plan_execute_cascade_frames_stream_timed.argtypes = cascade_frames + [vp, kp] + state + [vp] + report
    L.rf_var2_plan_cascade_frames_stream_num_kernels.argtypes = [vp, ctypes.c_int]
    L.rf_var2_plan_cascade_frames_stream_state_bytes.argtypes = [vp, ctypes.c_int, ctypes.c_int64]
    L.rf_var2_plan_cascade_frames_stream_state_bytes.restype = ctypes.c_size_t
    grad_state = [vp, vp, vp, ctypes.c_int64]      # state_in, grad_state_out, grad_state_in, state_stride
    L.rf_var2_plan_backward_cascade_frames_stream.argtypes = cascade_frames + [kp, vp, vp, vp, sp] + grad_state + [vp]
    L.rf_var2_plan_backward_cascade_frames_stream_timed.argtypes = cascade_frames + [kp, vp, vp, vp, sp] + grad_state + [vp] + report
    L.rf_var2_plan_backward_cascade_frames_stream_num_kernels.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.rf_last_error_string.restype = ctypes.c_char_p
    L.rf_version.restype = ctypes.c_char_p
    _lib = L
    return L


def check(status: int) -> None:
    if status != RF_OK:
        raise RecFilterError(status, lib().rf_last_error_string().decode())


def _timed(call, n: int):
    """[(kernel name, ms), ...] of a *_timed entry point with `n` launches: call(ms, names, n) returns its status"""
    ms = (ctypes.c_float * max(n, 1))()
    names = (ctypes.c_char_p * max(n, 1))()
    check(call(ms, names, n))
    return [(names[i].decode(), float(ms[i])) for i in range(n)]


class _PlanHandle:
    """the lifetime of the library's plan behind self._h; `_destroy` names the entry point that frees it"""
    _destroy = ""

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            getattr(lib(), self._destroy)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def _stream(stream) -> ctypes.c_void_p:
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return ctypes.c_void_p(s.cuda_stream)
