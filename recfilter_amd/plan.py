"""Plan: thin Python handle over rf_plan_* (include/recfilter_amd.h).

Images are torch CUDA(HIP) tensors used purely as device memory: a tensor of shape
(..., z, y, x), C-contiguous, is the reference's dense x-fastest buffer
(/root/reference lib/recfilter.cpp:969-981).  All arithmetic happens in the HIP kernels.
"""
from __future__ import annotations

import collections
import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import capi

Scan = Tuple[int, bool, Sequence[float]]   # (dim, causal, [feedfwd, fb1..fbk]); dim 0 = x

# rf_filter_desc.flags of plans created without an explicit `flags`.  0 as shipped.  tests/conftest.py sets
# capi.RF_PLAN_TILED_ONLY: most parity tests use small shapes on purpose and mean the TILED kernels when they ask for the
# automatic path (which sends images up to 1024^2 to the line kernels); tests/test_shipped_defaults.py resets it to 0.
DEFAULT_FLAGS = 0

_NP_DTYPES = {np.dtype(np.float32): capi.RF_F32, np.dtype(np.float64): capi.RF_F64,
              np.dtype(np.int32): capi.RF_I32, np.dtype(np.int16): capi.RF_I16, np.dtype(np.float16): capi.RF_F16}
# the numpy type of the planes of every pixel type that has one (numpy has no bfloat16: such a plan is keyed on the torch type)
_CODE_NP = {code: dt for dt, code in _NP_DTYPES.items()}
_TORCH_NAMES = {"float32": capi.RF_F32, "float64": capi.RF_F64, "int32": capi.RF_I32, "int16": capi.RF_I16,
                "float16": capi.RF_F16, "bfloat16": capi.RF_BF16}


def _dtype_code(dtype) -> int:
    """rf_dtype of a numpy / torch pixel type.  torch.float16 / np.float16 and torch.bfloat16 are STORAGE types: the planes
    hold 16-bit floats, the filter runs in f32 and rounds once at the final store (include/recfilter_amd.h, rf_dtype)."""
    try:
        import torch
        if isinstance(dtype, torch.dtype):
            name = str(dtype).replace("torch.", "")
            if name not in _TORCH_NAMES:
                raise TypeError(f"unsupported pixel type {dtype}")
            return _TORCH_NAMES[name]
    except ImportError:  # pragma: no cover
        pass
    dt = np.dtype(dtype)
    if dt not in _NP_DTYPES:
        raise TypeError(f"unsupported pixel type {dt}")
    return _NP_DTYPES[dt]


def _is_uint8(dtype) -> bool:
    """np.uint8 / torch.uint8 (or anything numpy reads as an unsigned byte)"""
    if dtype is None:
        return False
    try:
        return np.dtype(str(dtype).replace("torch.", "") if hasattr(dtype, "is_floating_point") else dtype) == np.dtype(np.uint8)
    except TypeError:
        return False


def _torch_dtype(code: int):
    import torch
    return {capi.RF_F32: torch.float32, capi.RF_F64: torch.float64, capi.RF_I32: torch.int32, capi.RF_I16: torch.int16,
            capi.RF_F16: torch.float16, capi.RF_BF16: torch.bfloat16}[code]


class Plan(capi._PlanHandle):
    """One tiled (or untiled) recursive filter on one device: rf_plan_create .. rf_plan_destroy."""
    _destroy = "rf_plan_destroy"

    def __init__(self, shape: Sequence[int], scans: Sequence[Scan], dtype=np.float32, clamped: bool = False,
                 planes: int = 1, tile: Optional[Sequence[int]] = None, path: int = capi.RF_PATH_AUTO,
                 device: int = -1, shard_rank: int = 0, shard_world: int = 1, shard_extents: Optional[Sequence[int]] = None,
                 prologue: Optional[Tuple[float, float]] = None,
                 epilogue: Optional[Tuple[float, float, float]] = None, input_dtype=None, flags: Optional[int] = None,
                 output_dtype=None):
        """prologue = (scale, bias): x' = scale*in + bias before the first scan;
        epilogue = (w_filtered, w_input, bias): out = w_filtered*F(x') + w_input*x' + bias
        (rf_pointwise_desc; fused into pass 1 / pass 2 on the fused path).  input_dtype=np.uint8 (with dtype float32):
        the input planes are unsigned bytes converted on load (rf_pointwise_desc.in_dtype = RF_IN_U8).
        output_dtype=np.uint8 (with input_dtype=np.uint8 and dtype float32; np.uint8 or torch.uint8 for either): the output
        planes are unsigned bytes too, out = sat8(f32 result), converted once at the final store (RF_IO_U8).
        flags: rf_filter_desc.flags (capi.RF_PLAN_*); None = recfilter_amd.plan.DEFAULT_FLAGS (0 as shipped)."""
        L = capi.lib()
        shape = tuple(int(s) for s in shape)
        if not 1 <= len(shape) <= capi.RF_MAX_DIMS:
            raise ValueError(f"1..{capi.RF_MAX_DIMS} dimensions supported, got shape {shape}")
        scans = list(scans)
        self._scan_arr = (capi.ScanDesc * max(len(scans), 1))()
        for i, (dim, causal, coeff) in enumerate(scans):
            coeff = [float(c) for c in coeff]
            if len(coeff) < 2:
                # lib/recfilter.cpp:274-278
                raise ValueError("cannot add a scan without feed forward and feedback coefficients")
            if len(coeff) - 1 > capi.RF_MAX_ORDER:
                raise ValueError(f"filter order {len(coeff) - 1} exceeds RF_MAX_ORDER={capi.RF_MAX_ORDER}")
            s = self._scan_arr[i]
            s.dim, s.causal, s.order, s.feedfwd = int(dim), int(bool(causal)), len(coeff) - 1, coeff[0]
            for j, c in enumerate(coeff[1:]):
                s.feedback[j] = c
        d = capi.FilterDesc()
        d.abi = capi.RF_ABI
        d.ndim = len(shape)
        for i, e in enumerate(reversed(shape)):      # numpy (z,y,x) -> extent[0] = x
            d.extent[i] = e
        d.dtype = _dtype_code(dtype)
        d.n_planes = int(planes)
        d.border = capi.RF_BORDER_CLAMP if clamped else capi.RF_BORDER_ZERO
        d.n_scans = len(scans)
        d.scans = ctypes.cast(self._scan_arr, ctypes.POINTER(capi.ScanDesc))
        if tile is not None:
            tile = list(tile)
            if len(tile) != len(shape):
                raise ValueError("tile needs one entry per dimension, in (x, y, z) order")
            for i, t in enumerate(tile):
                d.tile[i] = int(t)
        d.path = int(path)
        d.device = int(device)
        d.shard_rank, d.shard_world = int(shard_rank), int(shard_world)
        if shard_extents is not None:
            # rf_filter_desc.shard_extents: the extent of every rank's slab along the outermost dimension
            if len(shard_extents) != int(shard_world):
                raise ValueError("shard_extents needs one extent per rank")
            self._shard_extents = (ctypes.c_int64 * int(shard_world))(*[int(e) for e in shard_extents])
            d.shard_extents = ctypes.cast(self._shard_extents, ctypes.POINTER(ctypes.c_int64))
        if prologue is not None:
            d.pointwise.flags |= capi.RF_POINTWISE_PRE
            d.pointwise.pre_scale, d.pointwise.pre_bias = float(prologue[0]), float(prologue[1])
        if epilogue is not None:
            d.pointwise.flags |= capi.RF_POINTWISE_POST
            d.pointwise.post_filtered, d.pointwise.post_input, d.pointwise.post_bias = (float(v) for v in epilogue)
        self.input_np_dtype = self.output_np_dtype = None
        if output_dtype is not None:
            if not _is_uint8(output_dtype):
                raise TypeError(f"unsupported output type {output_dtype}: byte planes (uint8) or the pixel type")
            if not _is_uint8(input_dtype) or d.dtype != capi.RF_F32:
                raise TypeError("output_dtype=uint8 needs input_dtype=uint8 and dtype float32")
            self.output_np_dtype = np.dtype(np.uint8)
        if _is_uint8(input_dtype):
            d.pointwise.in_dtype = capi.RF_IO_U8 if self.output_np_dtype is not None else capi.RF_IN_U8
            self.input_np_dtype = np.dtype(np.uint8)
        elif input_dtype is not None and _dtype_code(input_dtype) != d.dtype:
            raise TypeError(f"unsupported input type {input_dtype} for pixel type {dtype}")
        d.flags = int(DEFAULT_FLAGS if flags is None else flags)
        self._desc = d
        self.shape = shape
        self.n_scans = len(scans)
        self.planes = int(planes)
        self.np_dtype = _CODE_NP.get(d.dtype)        # None for bfloat16, which numpy does not have
        self.dtype_code = int(d.dtype)
        self.shard_world = int(shard_world)
        self._h = ctypes.c_void_p()
        capi.check(L.rf_plan_create(ctypes.byref(d), ctypes.byref(self._h)))

    # -- queries ----------------------------------------------------------------------------
    @property
    def path(self) -> int:
        return capi.lib().rf_plan_path(self._h)

    @property
    def path_name(self) -> str:
        return capi.PATH_NAMES.get(self.path, "?")

    @property
    def tiles(self) -> Tuple[int, ...]:
        t = (ctypes.c_int32 * capi.RF_MAX_DIMS)()
        capi.check(capi.lib().rf_plan_tiles(self._h, t))
        return tuple(t[: len(self.shape)])

    @property
    def workspace_bytes(self) -> int:
        return int(capi.lib().rf_plan_workspace_bytes(self._h))

    @property
    def num_instances(self) -> int:
        """execution instances the plan holds: 1 + the replicas concurrent executes on other streams made it build"""
        return int(capi.lib().rf_plan_num_instances(self._h))

    @property
    def num_kernels(self) -> int:
        return int(capi.lib().rf_plan_num_kernels(self._h))

    @property
    def num_exchanges(self) -> int:
        return int(capi.lib().rf_plan_num_exchanges(self._h))

    def table(self, name: str) -> np.ndarray:
        n = ctypes.c_size_t()
        capi.check(capi.lib().rf_plan_table(self._h, name.encode(), None, 0, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.float64)
        capi.check(capi.lib().rf_plan_table(self._h, name.encode(),
                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n.value, None))
        return out

    # -- debugging aids ---------------------------------------------------------------------
    def debug_buffers(self) -> List[Tuple[int, str, int]]:
        """[(index, kind, bytes)] of every device buffer an execute of the plan's first instance uses, child plans included
        (rf_plan_debug_buffer / rf_plan_debug_buffer_kind); kind is "table", "zeroed" or "scratch".  A host-only plan lists
        what it would have allocated."""
        L, out, i = capi.lib(), [], 0
        n, kind = ctypes.c_size_t(), ctypes.c_int()
        while L.rf_plan_debug_buffer(self._h, i, None, ctypes.byref(n)) == capi.RF_OK:
            capi.check(L.rf_plan_debug_buffer_kind(self._h, i, ctypes.byref(kind)))
            out.append((i, capi.BUFFER_KIND_NAMES[kind.value], int(n.value)))
            i += 1
        return out

    def debug_fill(self, index: int, byte: int, stream=None) -> None:
        """rf_plan_debug_fill: every byte of buffer `index` becomes `byte`, on `stream` (default: torch's current stream).
        Raises for a table.  Scratch may hold anything before an execute; a zeroed buffer filled with non-zero bytes breaks
        the plan."""
        host_only = self._desc.device == capi.RF_DEVICE_HOST_ONLY       # (refused by the library; there is no stream to ask torch for)
        capi.check(capi.lib().rf_plan_debug_fill(self._h, int(index), int(byte), ctypes.c_void_p() if host_only else self._stream(stream)))

    # -- execution --------------------------------------------------------------------------
    def _pointers(self, tensors, inputs: bool = False) -> ctypes.Array:
        if len(tensors) != self.planes:
            raise ValueError(f"expected {self.planes} planes, got {len(tensors)}")
        arr = (ctypes.c_void_p * self.planes)()
        for i, t in enumerate(tensors):
            if tuple(t.shape) != self.shape:
                raise ValueError(f"plane {i}: shape {tuple(t.shape)} != plan shape {self.shape}")
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("planes must be contiguous device tensors")
            if inputs and self.input_np_dtype is not None:
                import torch
                if t.dtype != torch.uint8:
                    raise TypeError(f"plane {i}: the plan expects unsigned-byte input planes, got {t.dtype}")
            elif not inputs and self.output_np_dtype is not None:
                import torch
                if t.dtype != torch.uint8:
                    raise TypeError(f"plane {i}: the plan writes unsigned-byte output planes, got {t.dtype}")
            elif _dtype_code(t.dtype) != self._desc.dtype:
                raise TypeError(f"plane {i}: dtype {t.dtype} does not match the plan")
            arr[i] = t.data_ptr()
        return arr

    def _new_outputs(self, inputs):
        import torch
        tdt = torch.uint8 if self.output_np_dtype is not None else _torch_dtype(self.dtype_code)
        return [torch.empty(t.shape, dtype=tdt, device=t.device) for t in inputs]

    def execute(self, inputs, outputs=None, stream=None):
        """rf_plan_execute: asynchronous on `stream` (default: torch's current stream).  Executes on distinct streams may
        overlap: the plan runs them on replicas of itself with their own workspaces (include/recfilter_amd.h)."""
        import torch
        if outputs is None:
            outputs = self._new_outputs(inputs)
        pin, pout = self._pointers(inputs, True), self._pointers(outputs)
        capi.check(capi.lib().rf_plan_execute(self._h, pin, pout, self._stream(stream)))
        return outputs

    def execute_timed(self, inputs, outputs=None, stream=None):
        """rf_plan_execute_timed: returns (outputs, [(kernel name, ms), ...]) measured with HIP events."""
        import torch
        if outputs is None:
            outputs = self._new_outputs(inputs)
        pin, pout, s = self._pointers(inputs, True), self._pointers(outputs), self._stream(stream)
        return outputs, capi._timed(lambda *report: capi.lib().rf_plan_execute_timed(self._h, pin, pout, s, *report), self.num_kernels)

    # -- backward (rf_plan_backward) ------------------------------------------------------------
    def _backward_arguments(self, grad_outs, grad_ins, inputs, coeff_grads, stream):
        import torch
        grad_outs = list(grad_outs)
        if coeff_grads and inputs is None:
            raise ValueError("coefficient gradients need the inputs of the execute (inputs=...)")
        if not coeff_grads and inputs is not None:
            raise ValueError("inputs are read only for coefficient gradients: pass coeff_grads=True, or leave inputs out")
        if grad_ins is None:
            grad_ins = [torch.empty_like(g) for g in grad_outs]
        pgo, pgi = self._pointers(grad_outs), self._pointers(grad_ins)
        pin = self._pointers(list(inputs)) if coeff_grads else None
        coeffs = None
        if coeff_grads:
            coeffs = torch.empty((self.n_scans, 1 + capi.RF_MAX_ORDER), dtype=torch.float64, device=grad_outs[0].device)
        pc = ctypes.c_void_p(coeffs.data_ptr()) if coeffs is not None else None
        return pin, pgo, pgi, pc, grad_ins, coeffs, self._stream(stream)

    def backward(self, grad_outs, grad_ins=None, inputs=None, coeff_grads=False, stream=None):
        """rf_plan_backward: (grad_ins, coeffs) from grad_outs = dL/d(outputs) of an execute.  grad_ins = dL/d(inputs) (new
        tensors unless given; grad_ins[p] may be grad_outs[p]).  coeff_grads=True also returns `coeffs`, a device f64 tensor of
        shape (n_scans, 1 + RF_MAX_ORDER): row s = [dL/dfeedfwd, dL/dfeedback...] of scan s summed over the planes, zeros past
        the order; it needs `inputs`, the planes the execute read.  Otherwise coeffs is None and inputs must be left out.
        Asynchronous on `stream` (default: torch's current stream); nothing synchronises.  f32 planes, unsharded plans."""
        pin, pgo, pgi, pc, grad_ins, coeffs, s = self._backward_arguments(grad_outs, grad_ins, inputs, coeff_grads, stream)
        capi.check(capi.lib().rf_plan_backward(self._h, pin, pgo, pgi, pc, s))
        return grad_ins, coeffs

    def backward_timed(self, grad_outs, grad_ins=None, inputs=None, coeff_grads=False, stream=None):
        """rf_plan_backward_timed: (grad_ins, coeffs, [(launch name, ms), ...]) in execution order; synchronises the stream."""
        pin, pgo, pgi, pc, grad_ins, coeffs, s = self._backward_arguments(grad_outs, grad_ins, inputs, coeff_grads, stream)
        n = self.backward_num_kernels(coeff_grads)
        return grad_ins, coeffs, capi._timed(lambda *report: capi.lib().rf_plan_backward_timed(self._h, pin, pgo, pgi, pc, s, *report), n)

    def backward_num_kernels(self, coeff_grads: bool = False) -> int:
        """launches of one backward call (0 for a plan the backward refuses); the first query builds the child plans"""
        return int(capi.lib().rf_plan_backward_num_kernels(self._h, int(bool(coeff_grads))))

    def backward_workspace_bytes(self, coeff_grads: bool = False) -> int:
        """device memory the backward allocates on first need beyond its child plans' own tails and carries: 0 without
        coefficient gradients, (n_scans + 1) image sets and the reduction's slabs with them"""
        return int(capi.lib().rf_plan_backward_workspace_bytes(self._h, int(bool(coeff_grads))))

    def apply(self, inputs):
        """execute, out of place, as a differentiable torch operation: a tuple of `planes` output planes whose values are bit
        for bit execute's, differentiable with respect to the inputs (backward is `backward`).  No double backward."""
        inputs = list(inputs)
        if len(inputs) != self.planes:
            raise ValueError(f"expected {self.planes} planes, got {len(inputs)}")
        return _plan_function().apply(self, *inputs)

    # stepping API (sharded execution) ---------------------------------------------------------
    def begin(self, inputs, outputs, stream=None):
        pin, pout = self._pointers(inputs, True), self._pointers(outputs)
        capi.check(capi.lib().rf_plan_begin(self._h, pin, pout, self._stream(stream)))

    def exchange_bytes(self, i: int) -> int:
        return int(capi.lib().rf_plan_exchange_bytes(self._h, i))

    def exchange_local(self, i: int, send_ptr: int = 0) -> None:
        """Slab-local recurrence of exchange i; writes the slab's exit carry to the device buffer `send_ptr`."""
        capi.check(capi.lib().rf_plan_exchange_local(self._h, i, ctypes.c_void_p(send_ptr or None)))

    def exchange_apply(self, i: int, gathered_ptr: int) -> None:
        capi.check(capi.lib().rf_plan_exchange_apply(self._h, i, ctypes.c_void_p(gathered_ptr)))

    @property
    def has_interior(self) -> bool:
        return bool(capi.lib().rf_plan_has_interior(self._h))

    def interior(self) -> None:
        """rf_plan_interior: the work of this execute that does not depend on the exchange (the x/y stage of a z-sharded
        volume) -- call it between issuing the last all-gather and waiting for it."""
        capi.check(capi.lib().rf_plan_interior(self._h))

    def finish(self):
        capi.check(capi.lib().rf_plan_finish(self._h))

    def abort(self) -> None:
        """rf_plan_abort: abandon the execute this thread began and did not finish (a collective that raised)."""
        if self._h:
            capi.lib().rf_plan_abort(self._h)


# ---- coefficient design (lib/iir_coeff.cpp) ---------------------------------------------------
def gaussian_weights(sigma: float, order: int) -> List[float]:
    out = (ctypes.c_float * (order + 1))()
    capi.check(capi.lib().rf_gaussian_weights(float(sigma), int(order), out))
    return [float(v) for v in out]


def integral_image_coeff(n: int) -> List[float]:
    out = (ctypes.c_float * (n + 1))()
    capi.check(capi.lib().rf_integral_image_coeff(int(n), out))
    return [float(v) for v in out]


def overlap_feedback_coeff(a: Sequence[float], b: Sequence[float]) -> List[float]:
    fa, fb = (ctypes.c_float * len(a))(*a), (ctypes.c_float * len(b))(*b)
    out = (ctypes.c_float * (len(a) + len(b)))()
    capi.check(capi.lib().rf_overlap_feedback_coeff(fa, len(a), fb, len(b), out))
    return [float(v) for v in out]


def gaussian_box_filter(k: int, sigma: float) -> int:
    w = ctypes.c_int()
    capi.check(capi.lib().rf_gaussian_box_filter(int(k), float(sigma), ctypes.byref(w)))
    return int(w.value)


def box_difference(table, radius: int, order: Sequence[int], out=None, stream=None):
    """rf_box_difference: finite differences that turn a (higher-order) summed-area table into an iterated box filter
    (apps/box/box_filter.h).  `table` is a device tensor (..., y, x); `order` is per dimension in (x, y, z) order."""
    import torch
    if out is None:
        out = torch.empty_like(table)
    shape = tuple(table.shape)
    ext = (ctypes.c_int64 * len(shape))(*reversed(shape))
    order = list(order) + [0] * (len(shape) - len(order))
    ords = (ctypes.c_int32 * len(shape))(*order[:len(shape)])
    if not table.is_cuda or not table.is_contiguous() or not out.is_contiguous():
        raise ValueError("box_difference needs contiguous device tensors")
    if _dtype_code(table.dtype) in (capi.RF_F16, capi.RF_BF16):
        raise TypeError("box_difference takes f32 / f64 tables: differences of a table rounded to 16 bits are not a box filter")
    capi.check(capi.lib().rf_box_difference(ctypes.c_void_p(table.data_ptr()), ctypes.c_void_p(out.data_ptr()), len(shape), ext,
                                            _dtype_code(table.dtype), int(radius), ords, Plan._stream(stream)))
    return out


def tap_filter(inputs, taps, out=None, stream=None):
    """rf_tap_filter: out(p) = sum_t weight_t * inputs[plane_t](clamp(p + offset_t)) -- the clamped difference operators
    the reference's apps put behind a summed-area table (apps/DoG/diff_gauss.cpp:176-197).  `inputs` are device tensors
    of one shape and floating-point type; `taps` is a list of (plane, offset, weight) with offset in (x, y, z) order."""
    import torch
    inputs = list(inputs)
    if out is None:
        out = torch.empty_like(inputs[0])
    shape = tuple(inputs[0].shape)
    for t in inputs + [out]:
        if not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape or t.dtype != inputs[0].dtype:
            raise ValueError("tap_filter needs contiguous device tensors of one shape and type")
    if _dtype_code(inputs[0].dtype) in (capi.RF_F16, capi.RF_BF16):
        raise TypeError("tap_filter takes f32 / f64 planes, not 16-bit float planes")
    nd = len(shape)
    ext = (ctypes.c_int64 * nd)(*reversed(shape))
    arr = (capi.Tap * len(taps))()
    for i, (plane, offset, weight) in enumerate(taps):
        arr[i].plane, arr[i].weight = int(plane), float(weight)
        offset = list(offset) + [0] * (capi.RF_MAX_DIMS - len(offset))
        for d in range(capi.RF_MAX_DIMS):
            arr[i].offset[d] = int(offset[d])
    ptrs = (ctypes.c_void_p * len(inputs))(*[t.data_ptr() for t in inputs])
    capi.check(capi.lib().rf_tap_filter(ptrs, len(inputs), ctypes.c_void_p(out.data_ptr()), nd, ext, _dtype_code(inputs[0].dtype),
                                        arr, len(taps), Plan._stream(stream)))
    return out


def stream_copy_ms(src, dst, reps: int = 5, stream=None) -> float:
    """rf_stream_copy timed with HIP events on `stream` (the current stream by default): milliseconds per copy of the f32
    image `src` (rows x width, whole 256 x 128 tiles) into `dst`, mean of `reps` after one untimed copy.  The measured
    ceiling of a read-once / write-once pass in the final pass's access shape (bench.py: roofline.copy_ceiling_gbps)."""
    import torch
    if src.dtype != torch.float32 or dst.dtype != torch.float32 or src.dim() < 2 or src.shape != dst.shape or not (src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("stream_copy_ms needs two contiguous f32 device tensors of one shape")
    width, rows = int(src.shape[-1]), int(src.numel() // src.shape[-1])
    st = torch.cuda.current_stream() if stream is None else stream
    h = ctypes.c_void_p(st.cuda_stream)
    call = lambda: capi.check(capi.lib().rf_stream_copy(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), width, rows, h))
    call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        e0.record(st)
        for _ in range(reps):
            call()
        e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def second_order_sections(coeff: Sequence[float]) -> List[List[float]]:
    """Factors one scan {b, a1..ak} (y[i] = b x[i] + sum_j a_j y[i-j-1]) into first/second-order scans with the same
    transfer function: the poles (roots of z^k - a1 z^(k-1) - ... - ak) are paired into conjugate pairs / pairs of real
    poles, b goes to the first section.  Applied one after the other in the same direction with a ZERO border the
    sections reproduce the original scan exactly (up to rounding); this is how orders above 3 reach the fused kernels
    (the reference's audio apps sweep orders up to 29, apps/audio/audio_filter_high_order.cpp).  The inverse of
    overlap_feedback_coeff (lib/iir_coeff.cpp:236-263).  Numerically this is a cascade form: well conditioned for
    the usual low-pass designs (order-3 Gaussian: 3e-7), but for polynomials whose poles sit evenly on a circle (that
    app's dummy coefficients) f32 cascades lose accuracy quickly above order 15 -- use f64 pixels or the direct form
    there."""
    coeff = [float(c) for c in coeff]
    k = len(coeff) - 1
    if k <= 2:
        return [coeff]
    poles = np.roots([1.0] + [-c for c in coeff[1:]])
    cplx = sorted([p for p in poles if p.imag > 1e-12 * max(1.0, abs(p))], key=lambda p: -abs(p))
    real = sorted([p.real for p in poles if abs(p.imag) <= 1e-12 * max(1.0, abs(p))], key=lambda p: -abs(p))
    sections = [[1.0, float(2.0 * p.real), float(-(abs(p) ** 2))] for p in cplx]
    while len(real) >= 2:
        p, q = real.pop(0), real.pop(0)
        sections.append([1.0, float(p + q), float(-p * q)])
    if real:
        sections.append([1.0, float(real[0])])
    sections[0][0] = coeff[0]
    return sections


# ---- torch.autograd ---------------------------------------------------------------------------
_function = None
_filter_function = None


def _plan_function():
    """the torch.autograd.Function behind Plan.apply (torch is imported when it is first needed)"""
    global _function
    if _function is not None:
        return _function
    import torch

    class PlanFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, *inputs):
            ctx.plan = plan
            return tuple(plan.execute([t.contiguous() for t in inputs]))

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, *grad_outs):
            with torch.cuda.device(grad_outs[0].device):
                grad_ins, _ = ctx.plan.backward([g.contiguous() for g in grad_outs])
            return (None, *[g if n else None for g, n in zip(grad_ins, ctx.needs_input_grad[1:])])

    _function = PlanFunction
    return _function


FILTER_PLAN_CACHE = 16       # plans recursive_filter keeps (least recently used first out)
_filter_plans: "collections.OrderedDict[tuple, Plan]" = collections.OrderedDict()


def _filter_plan(key) -> Plan:
    """the cached plan of `key` = (shape, device index, clamped, ((dim, causal, (coefficients...)), ...)); a plan that falls
    out of the cache is destroyed"""
    plan = _filter_plans.get(key)
    if plan is not None and plan._h:
        _filter_plans.move_to_end(key)
        return plan
    shape, device, clamped, scans = key
    plan = Plan(shape, [(d, c, list(w)) for d, c, w in scans], clamped=clamped, device=device)
    _filter_plans[key] = plan
    while len(_filter_plans) > FILTER_PLAN_CACHE:
        _, old = _filter_plans.popitem(last=False)
        old.close()
    return plan


def _recursive_filter_function():
    global _filter_function
    if _filter_function is not None:
        return _filter_function
    import torch

    class RecursiveFilterFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, key, image, *coeffs):
            image = image.contiguous()
            ctx.key = key
            ctx.coeffs = [(c.shape, c.dtype, c.device) for c in coeffs]
            ctx.save_for_backward(image)
            with torch.cuda.device(image.device):
                return _filter_plan(key).execute([image])[0]

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            (image,) = ctx.saved_tensors
            want = any(ctx.needs_input_grad[2:])
            with torch.cuda.device(image.device):
                plan = _filter_plan(ctx.key)           # (built again if the cache dropped it meanwhile)
                if want:
                    grad_ins, rows = plan.backward([grad_out.contiguous()], inputs=[image], coeff_grads=True)
                else:
                    grad_ins, rows = plan.backward([grad_out.contiguous()])
            grads = [None] * len(ctx.coeffs)
            for s, ((shape, dtype, device), need) in enumerate(zip(ctx.coeffs, ctx.needs_input_grad[2:])):
                if need:
                    grads[s] = rows[s, :shape[0]].to(device=device, dtype=dtype)
            return (None, grad_ins[0] if ctx.needs_input_grad[1] else None, *grads)

    _filter_function = RecursiveFilterFunction
    return _filter_function


def recursive_filter(image, scans, coeffs, clamped: bool = False):
    """The recursive filter `scans` = [(dim, causal), ...] (dim 0 = x, the last axis) of the f32 device tensor `image` (1 to 3
    dimensions), scan s with the coefficients coeffs[s] = a 1-D tensor [feedfwd, fb1 .. fbk]: differentiable with respect to
    the image and to every coefficient tensor.  One tensor object may appear several times in `coeffs` (the four scans of a
    Gaussian): autograd sums its rows.  The values are a Plan's execute; backward is Plan.backward (no double backward).
    Plans are cached by shape, device, border and coefficient VALUES in a least-recently-used cache of FILTER_PLAN_CACHE plans;
    a plan that falls out is destroyed.  Reading the coefficient values from device tensors SYNCHRONISES with the device on
    every call (a plan turns its coefficients into tables on the host); keep the coefficients on the host where that matters.
    Calls that share a plan are ordered by the caller (one stream)."""
    import torch
    scans, coeffs = list(scans), list(coeffs)
    if len(scans) != len(coeffs):
        raise ValueError(f"{len(scans)} scans need {len(scans)} coefficient tensors, got {len(coeffs)}")
    if not image.is_cuda or image.dtype != torch.float32:
        raise TypeError("recursive_filter takes an f32 device tensor")
    values = []
    for s, c in enumerate(coeffs):
        if not torch.is_tensor(c) or c.dim() != 1 or c.numel() < 2 or not c.is_floating_point():
            raise ValueError(f"coeffs[{s}]: a 1-D floating-point tensor [feedfwd, fb1 .. fbk] is needed")
        values.append(tuple(float(np.float32(v)) for v in c.detach().cpu().tolist()))
    key = (tuple(image.shape), image.device.index, bool(clamped),
           tuple((int(d), bool(c), v) for (d, c), v in zip(scans, values)))
    return _recursive_filter_function().apply(key, image, *coeffs)
