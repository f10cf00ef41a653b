"""Spatially varying first-order scans: thin Python handle over rf_var_plan_* (include/recfilter_amd.h), and the
edge-aware smoothing built on them (the domain-transform recursive filter of Gastal & Oliveira 2011).

The scans run in the HIP kernels of kernels_var.hip; torch tensors are device memory.  Two forms of the filter:
  planes   `domain_transform_weights` computes a pair of weight planes per iteration with torch (a pointwise expression of the
           guide image, on the guide's device); `VarPlan.execute` reads them.
  power    `domain_transform_distances` (rf_var_distances, one HIP launch) gives the two exponent planes all iterations share;
           `VarPlan.execute_power` forms w = a_k ** d in the scan kernels.  Nothing but the scans' output is stored.
  plan     `SmoothPlan` (rf_smooth_plan_*): the power form as one object of the library, which owns the distance planes and
           sequences every launch; f32 or uint8 images (bytes in, bytes out, no conversion pass).

Volumes: `VarPlan.volume`, `var_scan_volume`, `domain_transform_distances_volume`, `SmoothPlan.volume` and
`edge_aware_smooth_volume` are the same on (D, H, W) volumes with scans along x, y and z (rf_var_plan_create_volume,
rf_var_distances_volume, rf_smooth_plan_create_volume).  `domain_transform_distances_volume_backward`
(rf_var_distances_volume_backward) is the adjoint of the volume distances for f32 guides.  The smoothing plan of a volume has a
backward where it is asked for: `SmoothPlan.volume(..., differentiable=True)` (RF_SMOOTH_VOLUME_BACKWARD, f32 volumes) gives
`backward`, `backward_timed` and `apply` -- 1 + 18 K launches with the distances held constant, 51 K - 7 through them -- and
`edge_aware_smooth_volume(..., differentiable=True)` goes through it; without the flag the backward is refused as before.

The plane form is differentiable: `VarPlan.backward` (rf_var_plan_backward) is the adjoint of `VarPlan.execute` in the same HIP
kernels' adjoint instances -- gradients with respect to the image planes and, where asked for, the weight planes -- and
`VarPlan.apply` / `var_scan` put it behind torch.autograd.  So are the power form and the plan: `VarPlan.backward_power`
(rf_var_plan_backward_power; gradients with respect to the image planes and the exponent planes), `domain_transform_distances_backward`
(rf_var_distances_backward; the guide's gradient from those of the two distance planes) and `SmoothPlan.backward`
(rf_smooth_plan_backward: both, sequenced by the library), behind `VarPlan.apply_power`, `SmoothPlan.apply` and
`edge_aware_smooth(form="plan", differentiable=True)`.  f32 planes only; no byte-guide gradient; no double backward.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Sequence, Tuple

from . import capi
from .capi import _PlanHandle, _timed

VarScan = Tuple[int, bool, int]      # (dim, causal, index of the weight plane); dim 0 = x


def _aligned_contiguous(t):
    """what the library takes: contiguous, 16-byte aligned"""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _plane_pointer(t, shape, dtype, dtype_text: str, what: str) -> int:
    """the address of one plane, after the checks every plane of a call gets"""
    if tuple(t.shape) != shape:
        raise ValueError(f"{what}: shape {tuple(t.shape)} != plan shape {shape}")
    if t.dtype != dtype:
        raise TypeError(f"{what}: {dtype_text} planes only, got {t.dtype}")
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("planes must be contiguous device tensors")
    return t.data_ptr()


def _host_only_nulls(plan, *counts):
    """None -- or, for a host-only plan, which the library refuses to run (there are no device tensors to take pointers from, and no
    stream): a null pointer array for every count, None where the count is None"""
    if plan._desc.device != capi.RF_DEVICE_HOST_ONLY:
        return None
    return [None if n is None else (ctypes.c_void_p * max(n, 1))() for n in counts]


def _device_index(t) -> int:
    import torch
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


class VarPlan(_PlanHandle):
    """A list of at most capi.RF_VAR_MAX_SCANS scans  y[i] = (1 - w[i]) x[i] + w[i] y[i-1]  (causal; the anticausal one couples
    sample i to i+1 through w[i+1]) over `planes` f32 planes of `shape` = (height, width) that share `n_weights` weight planes.
    Element 0 of a weight plane along the scanned dimension is never used.  One plan owns one workspace: order its executes."""
    _destroy = "rf_var_plan_destroy"

    def __init__(self, shape: Sequence[int], scans: Sequence[VarScan], planes: int = 1, n_weights: int = 1, device: int = -1):
        shape = tuple(int(s) for s in shape)
        if not 1 <= len(shape) <= capi.RF_MAX_DIMS:
            raise ValueError(f"1..{capi.RF_MAX_DIMS} dimensions, got shape {shape}")
        d = capi.VarDesc()
        d.ndim = len(shape)
        for i, e in enumerate(reversed(shape)):      # (y, x) -> extent[0] = x
            d.extent[i] = e
        self._create("rf_var_plan_create", d, shape, scans, planes, n_weights, device)

    def _create(self, create: str, d, shape, scans, planes, n_weights, device) -> "VarPlan":
        """what the three kinds of plan share: the scan array, the common fields of the description `d` (which holds its kind's own
        already), the attributes, and the call of the library's `create`"""
        scans = list(scans)
        self._scan_arr = (capi.VarScanDesc * max(len(scans), 1))()
        for i, (dim, causal, weights) in enumerate(scans):
            s = self._scan_arr[i]
            s.dim, s.causal, s.weights = int(dim), int(bool(causal)), int(weights)
        d.abi = capi.RF_ABI
        d.dtype = capi.RF_F32
        d.n_planes, d.n_weights = int(planes), int(n_weights)
        d.n_scans = len(scans)
        d.scans = ctypes.cast(self._scan_arr, ctypes.POINTER(capi.VarScanDesc))
        d.device = int(device)
        d.flags = 0
        self._desc = d
        self.shape, self.planes, self.n_weights = shape, int(planes), int(n_weights)
        self.scans = [(int(dim), bool(causal), int(weights)) for dim, causal, weights in scans]
        self._h = ctypes.c_void_p()
        capi.check(getattr(capi.lib(), create)(ctypes.byref(d), ctypes.byref(self._h)))
        return self

    @classmethod
    def signal(cls, length: int, scans: Sequence[VarScan], planes: int = 1, n_weights: int = 1, device: int = -1) -> "VarPlan":
        """rf_var_plan_create_signal: the plan of long 1-D signals -- `planes` dense f32 signals of `length` samples (a multiple
        of 4, up to 2**30) that share `n_weights` weight signals; every scan has dim 0.  `shape` is (length,), and every method
        works as on an image plan, a plane being a 1-D tensor.  A lane owns 64 samples, a wave 4096; the launches are
        var_tails_1d, var_carry_1d, var_pass2_1d per stage."""
        d = capi.VarSignalDesc()
        d.length = int(length)
        return cls.__new__(cls)._create("rf_var_plan_create_signal", d, (int(length),), scans, planes, n_weights, device)

    @classmethod
    def volume(cls, shape: Sequence[int], scans: Sequence[VarScan], planes: int = 1, n_weights: int = 1, device: int = -1) -> "VarPlan":
        """rf_var_plan_create_volume: the plan of `planes` dense f32 volumes of `shape` = (depth, height, width) that share
        `n_weights` weight volumes; dim 0 = x, 1 = y, 2 = z, and element 0 of a weight volume along the scanned axis is never
        used.  Every method works as on an image plan, a plane being a 3-D tensor.  An x or y stage takes all slices in one
        launch, each bit for bit what VarPlan((height, width)) gives on it; a z stage is bit for bit the y stage of the 2-D plan
        on the (depth, height * width) reshaped volume.  Three launches per stage whatever the depth (var_tails_z, var_carry,
        var_pass2_z for z).  width % 4 == 0, extents up to 2**21, height * width <= 2**30, depth * planes <= 65535."""
        shape = tuple(int(s) for s in shape)
        if len(shape) != 3:
            raise ValueError(f"shape must be (depth, height, width), got {shape}")
        d = capi.VarVolumeDesc()
        d.depth, d.height, d.width = shape
        return cls.__new__(cls)._create("rf_var_plan_create_volume", d, shape, scans, planes, n_weights, device)

    # -- queries ----------------------------------------------------------------------------
    @property
    def workspace_bytes(self) -> int:
        return int(capi.lib().rf_var_plan_workspace_bytes(self._h))

    @property
    def num_kernels(self) -> int:
        return int(capi.lib().rf_var_plan_num_kernels(self._h))

    # -- execution --------------------------------------------------------------------------
    def _pointers(self, tensors, count: int, what: str) -> ctypes.Array:
        import torch
        if len(tensors) != count:
            raise ValueError(f"expected {count} {what} planes, got {len(tensors)}")
        arr = (ctypes.c_void_p * count)()
        for i, t in enumerate(tensors):
            arr[i] = _plane_pointer(t, self.shape, torch.float32, "float32", f"{what} plane {i}")
        return arr

    def _arguments(self, ins, weights, outs, stream):
        """(input, weight and output pointers, the outputs, the stream's handle)"""
        import torch
        nulls = _host_only_nulls(self, self.planes, self.n_weights, self.planes)
        if nulls:
            return (*nulls, None, ctypes.c_void_p())
        if outs is None:
            outs = [torch.empty_like(t) for t in ins]
        return (self._pointers(ins, self.planes, "input"), self._pointers(weights, self.n_weights, "weight"),
                self._pointers(outs, self.planes, "output"), outs, self._stream(stream))

    def execute(self, ins, weights, outs=None, stream=None):
        """rf_var_plan_execute: asynchronous on `stream` (default: torch's current stream).  outs=None allocates the outputs;
        outs may be the inputs themselves (in place)."""
        pin, pw, pout, outs, s = self._arguments(ins, weights, outs, stream)
        capi.check(capi.lib().rf_var_plan_execute(self._h, pin, pw, pout, s))
        return outs

    def execute_timed(self, ins, weights, outs=None, stream=None):
        """rf_var_plan_execute_timed: (outputs, [(kernel name, ms), ...]) measured with HIP events; synchronises the stream."""
        pin, pw, pout, outs, s = self._arguments(ins, weights, outs, stream)
        return outs, _timed(lambda *report: capi.lib().rf_var_plan_execute_timed(self._h, pin, pw, pout, s, *report), self.num_kernels)

    def _bases(self, bases) -> ctypes.Array:
        bases = [float(b) for b in bases]
        if len(bases) != self.n_weights:
            raise ValueError(f"expected {self.n_weights} bases, got {len(bases)}")
        return (ctypes.c_float * self.n_weights)(*bases)

    def execute_power(self, ins, exponents, bases, outs=None, stream=None):
        """rf_var_plan_execute_power: as execute, but plane k of `exponents` holds d >= 0 and the scans use
        w = exp2(d * log2(bases[k])), formed in the kernels; 0 < bases[k] < 1, one per exponent plane."""
        pb = self._bases(bases)
        pin, pd, pout, outs, s = self._arguments(ins, exponents, outs, stream)
        capi.check(capi.lib().rf_var_plan_execute_power(self._h, pin, pd, pb, pout, s))
        return outs

    def execute_power_timed(self, ins, exponents, bases, outs=None, stream=None):
        """rf_var_plan_execute_power_timed: (outputs, [(kernel name, ms), ...]); the launches execute_timed names."""
        pb = self._bases(bases)
        pin, pd, pout, outs, s = self._arguments(ins, exponents, outs, stream)
        return outs, _timed(lambda *report: capi.lib().rf_var_plan_execute_power_timed(self._h, pin, pd, pb, pout, s, *report), self.num_kernels)

    # -- the adjoint ------------------------------------------------------------------------
    def backward_num_kernels(self, with_weights: bool = False) -> int:
        """rf_var_plan_backward_num_kernels: 3 launches per scan, 7 with weight gradients"""
        return int(capi.lib().rf_var_plan_backward_num_kernels(self._h, int(bool(with_weights))))

    def backward_workspace_bytes(self, with_weights: bool = False) -> int:
        """rf_var_plan_backward_workspace_bytes: what the first backward call with weight gradients allocates, beyond
        workspace_bytes: (scans + 1) * planes f32 planes; 0 without weight gradients"""
        return int(capi.lib().rf_var_plan_backward_workspace_bytes(self._h, int(bool(with_weights))))

    def _backward_arguments(self, ins, weights, grad_outs, grad_ins, grad_weights, stream):
        """(the five pointer arrays, grad_ins, grad_weights, the stream's handle)"""
        import torch
        nulls = _host_only_nulls(self, self.planes if ins is not None else None, self.n_weights, self.planes, self.planes,
                                 self.n_weights if grad_weights is not None else None)
        if nulls:
            return (*nulls, None, None, ctypes.c_void_p())
        if grad_ins is None:
            grad_ins = [torch.empty_like(t) for t in grad_outs]
        pgw = None
        if grad_weights is not None:
            if len(grad_weights) != self.n_weights:
                raise ValueError(f"expected {self.n_weights} entries in grad_weights (None: no gradient for that plane), got {len(grad_weights)}")
            pgw = (ctypes.c_void_p * self.n_weights)()
            for k, t in enumerate(grad_weights):
                if t is not None:
                    pgw[k] = self._pointers([t], 1, f"gradient of weight plane {k}:")[0]
        return (self._pointers(ins, self.planes, "input") if ins is not None else None, self._pointers(weights, self.n_weights, "weight"),
                self._pointers(grad_outs, self.planes, "grad_out"), self._pointers(grad_ins, self.planes, "grad_in"), pgw,
                grad_ins, grad_weights, self._stream(stream))

    def backward(self, ins, weights, grad_outs, grad_ins=None, grad_weights=None, stream=None):
        """rf_var_plan_backward, the adjoint of execute: (grad_ins, grad_weights) from grad_outs = dL/d(outs).  grad_ins=None
        allocates them; grad_ins may be grad_outs themselves (in place).  grad_weights: None (no weight gradient; `ins` may then
        be None too), or a list of n_weights entries, each a plane to be WRITTEN or None for a plane that needs no gradient; a
        plane no scan reads is left as it is.  Asynchronous on `stream` (default: torch's current stream); uses the plan's
        workspace like an execute."""
        pin, pw, pgo, pgi, pgw, grad_ins, grad_weights, s = self._backward_arguments(ins, weights, grad_outs, grad_ins, grad_weights, stream)
        capi.check(capi.lib().rf_var_plan_backward(self._h, pin, pw, pgo, pgi, pgw, s))
        return grad_ins, grad_weights

    def backward_timed(self, ins, weights, grad_outs, grad_ins=None, grad_weights=None, stream=None):
        """rf_var_plan_backward_timed: (grad_ins, grad_weights, [(kernel name, ms), ...]); synchronises the stream.  The var_grad
        launch of a weight plane without a gradient is skipped and reports 0 ms."""
        pin, pw, pgo, pgi, pgw, grad_ins, grad_weights, s = self._backward_arguments(ins, weights, grad_outs, grad_ins, grad_weights, stream)
        n = self.backward_num_kernels(grad_weights is not None and any(t is not None for t in grad_weights))
        return grad_ins, grad_weights, _timed(lambda *report: capi.lib().rf_var_plan_backward_timed(self._h, pin, pw, pgo, pgi, pgw, s, *report), n)

    def backward_power(self, ins, exponents, bases, grad_outs, grad_ins=None, grad_exponents=None, stream=None):
        """rf_var_plan_backward_power, the adjoint of execute_power: (grad_ins, grad_exponents).  As backward, with the exponent
        planes and their bases in the place of the weights; a gradient plane receives dL/dd = (w ln base) dL/dw."""
        pb = self._bases(bases)
        pin, pw, pgo, pgi, pgw, grad_ins, grad_exponents, s = self._backward_arguments(ins, exponents, grad_outs, grad_ins, grad_exponents, stream)
        capi.check(capi.lib().rf_var_plan_backward_power(self._h, pin, pw, pb, pgo, pgi, pgw, s))
        return grad_ins, grad_exponents

    def backward_power_timed(self, ins, exponents, bases, grad_outs, grad_ins=None, grad_exponents=None, stream=None):
        """rf_var_plan_backward_power_timed: (grad_ins, grad_exponents, [(kernel name, ms), ...]); the launches backward_timed names"""
        pb = self._bases(bases)
        pin, pw, pgo, pgi, pgw, grad_ins, grad_exponents, s = self._backward_arguments(ins, exponents, grad_outs, grad_ins, grad_exponents, stream)
        n = self.backward_num_kernels(grad_exponents is not None and any(t is not None for t in grad_exponents))
        return grad_ins, grad_exponents, _timed(lambda *report: capi.lib().rf_var_plan_backward_power_timed(self._h, pin, pw, pb, pgo, pgi, pgw, s, *report), n)

    # -- the gradient of the bases ---------------------------------------------------------------
    def backward_bases_num_kernels(self) -> int:
        """rf_var_plan_backward_bases_num_kernels: 7 launches per scan and one var_param_sum"""
        return int(capi.lib().rf_var_plan_backward_bases_num_kernels(self._h))

    def backward_bases_workspace_bytes(self) -> int:
        """rf_var_plan_backward_bases_workspace_bytes: backward_workspace_bytes(True) and the f64 slabs, one entry per workgroup of
        every var_grad launch"""
        return int(capi.lib().rf_var_plan_backward_bases_workspace_bytes(self._h))

    def _grad_bases(self, grad_bases, like):
        """(the buffer dL/dbases goes to -- a float64 device tensor of n_weights entries -- and its address)"""
        import torch
        if self._desc.device == capi.RF_DEVICE_HOST_ONLY:
            return None, ctypes.c_void_p()
        if grad_bases is None:
            grad_bases = torch.empty(self.n_weights, dtype=torch.float64, device=like.device)
        if grad_bases.dtype != torch.float64 or tuple(grad_bases.shape) != (self.n_weights,) or not grad_bases.is_cuda or not grad_bases.is_contiguous():
            raise ValueError(f"grad_bases must be a contiguous float64 device tensor of {self.n_weights} entries")
        return grad_bases, ctypes.c_void_p(grad_bases.data_ptr())

    def backward_power_bases(self, ins, exponents, bases, grad_outs, grad_ins=None, grad_exponents=None, grad_bases=None, stream=None):
        """rf_var_plan_backward_power_bases: (grad_ins, grad_exponents, grad_bases).  backward_power on its weight-gradient route --
        grad_exponents may be None or hold None entries, the planes that are given receive backward_power's bits -- and
        grad_bases, a float64 DEVICE tensor of n_weights entries (None allocates it), receives dL/dbases[k]: a streaming f64
        reduction without atomics, reproducible bit for bit.  Asynchronous: reading grad_bases on the host synchronises."""
        pb = self._bases(bases)
        pin, pw, pgo, pgi, pgw, grad_ins, grad_exponents, s = self._backward_arguments(ins, exponents, grad_outs, grad_ins, grad_exponents, stream)
        grad_bases, pgb = self._grad_bases(grad_bases, grad_ins[0] if grad_ins else None)
        capi.check(capi.lib().rf_var_plan_backward_power_bases(self._h, pin, pw, pb, pgo, pgi, pgw, pgb, s))
        return grad_ins, grad_exponents, grad_bases

    def backward_power_bases_timed(self, ins, exponents, bases, grad_outs, grad_ins=None, grad_exponents=None, grad_bases=None, stream=None):
        """rf_var_plan_backward_power_bases_timed: (grad_ins, grad_exponents, grad_bases, [(kernel name, ms), ...])"""
        pb = self._bases(bases)
        pin, pw, pgo, pgi, pgw, grad_ins, grad_exponents, s = self._backward_arguments(ins, exponents, grad_outs, grad_ins, grad_exponents, stream)
        grad_bases, pgb = self._grad_bases(grad_bases, grad_ins[0] if grad_ins else None)
        timings = _timed(lambda *report: capi.lib().rf_var_plan_backward_power_bases_timed(self._h, pin, pw, pb, pgo, pgi, pgw, pgb, s, *report),
                         self.backward_bases_num_kernels())
        return grad_ins, grad_exponents, grad_bases, timings

    def apply_power(self, ins, exponents, bases):
        """execute_power, out of place, as a differentiable torch operation: values bit for bit execute_power's.  Backward is
        `backward_power` -- the image gradient always, the gradient of an exponent plane where that plane requires one.  `bases`:
        a list of floats, which are constants -- or a float tensor of n_weights entries (any device), which receives a gradient
        where it requires one: backward is then `backward_power_bases`, and reading the tensor's values costs one host read per
        call.  No double backward."""
        import torch
        if len(ins) != self.planes or len(exponents) != self.n_weights:
            raise ValueError(f"expected {self.planes} input planes and {self.n_weights} exponent planes, got {len(ins)} and {len(exponents)}")
        if isinstance(bases, torch.Tensor):
            if not bases.is_floating_point() or bases.numel() != self.n_weights:
                raise ValueError(f"bases must be a float tensor of {self.n_weights} entries, got {bases.dtype} {tuple(bases.shape)}")
            values = [float(b) for b in bases.detach().reshape(-1).to(torch.float64).cpu().tolist()]
            return _var_scan_function().apply((self, values), *ins, *exponents, bases)
        bases = [float(b) for b in bases]
        if len(bases) != self.n_weights:
            raise ValueError(f"expected {self.n_weights} bases, got {len(bases)}")
        return _var_scan_function().apply((self, bases), *ins, *exponents)

    def apply(self, ins, weights):
        """execute, out of place, as a differentiable torch operation: a tuple of `planes` output planes whose values are bit for
        bit execute's.  Backward is `backward` -- the image gradient always, the gradient of a weight plane where that plane
        requires one.  Only the inputs and the weights are saved; no double backward."""
        if len(ins) != self.planes or len(weights) != self.n_weights:
            raise ValueError(f"expected {self.planes} input planes and {self.n_weights} weight planes, got {len(ins)} and {len(weights)}")
        return _var_scan_function().apply((self, None), *ins, *weights)


_function = None


def _var_scan_function():
    """the torch.autograd.Function behind VarPlan.apply (torch is imported when it is first needed)"""
    global _function
    if _function is not None:
        return _function
    import torch
    plane = _aligned_contiguous

    class VarScanFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan_and_bases, *tensors):      # bases None: the plane form; else the power form
            plan, bases = plan_and_bases
            ins = [plane(t) for t in tensors[:plan.planes]]
            weights = [plane(t) for t in tensors[plan.planes:plan.planes + plan.n_weights]]
            ctx.plan, ctx.bases = plan, bases
            # apply_power's bases tensor, where there is one: backward needs what its gradient looks like, not the tensor
            t = tensors[plan.planes + plan.n_weights] if len(tensors) > plan.planes + plan.n_weights else None
            ctx.bases_like = None if t is None else (t.shape, t.dtype, t.device)
            ctx.save_for_backward(*ins, *weights)
            return tuple(plan.execute(ins, weights) if bases is None else plan.execute_power(ins, weights, bases))

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, *grad_outs):
            plan = ctx.plan
            saved = ctx.saved_tensors
            ins, weights = list(saved[:plan.planes]), list(saved[plan.planes:])
            need_in = ctx.needs_input_grad[1:1 + plan.planes]
            need_w = ctx.needs_input_grad[1 + plan.planes:1 + plan.planes + plan.n_weights]
            need_bases = ctx.bases_like is not None and ctx.needs_input_grad[1 + plan.planes + plan.n_weights]
            read = {k for _, _, k in plan.scans}
            grad_weights = None
            if any(n and k in read for k, n in enumerate(need_w)):
                grad_weights = [torch.empty_like(w) if n and k in read else None for k, (w, n) in enumerate(zip(weights, need_w))]
            with torch.cuda.device(ins[0].device):
                grad_bases = None
                if ctx.bases is None:
                    grad_ins, grad_weights = plan.backward(ins, weights, [plane(g) for g in grad_outs], None, grad_weights)
                elif need_bases:
                    grad_ins, grad_weights, grad_bases = plan.backward_power_bases(ins, weights, ctx.bases, [plane(g) for g in grad_outs], None, grad_weights)
                else:
                    grad_ins, grad_weights = plan.backward_power(ins, weights, ctx.bases, [plane(g) for g in grad_outs], None, grad_weights)
            grad_weights = grad_weights or [None] * plan.n_weights
            # (a weight plane that no scan reads has a gradient of zero)
            grad_weights = [torch.zeros_like(w) if n and k not in read else g for k, (w, n, g) in enumerate(zip(weights, need_w, grad_weights))]
            grads = (None, *[g if n else None for g, n in zip(grad_ins, need_in)], *grad_weights)
            if ctx.bases_like is None:
                return grads
            shape, dtype, device = ctx.bases_like
            return (*grads, grad_bases.to(device=device, dtype=dtype).reshape(shape) if need_bases else None)

    _function = VarScanFunction
    return _function


# plans of the functional front ends, one cache per kind of plan, every one keyed (shape, scans, planes, n_weights, device)
_scan_plans: Dict[tuple, VarPlan] = {}
_volume_plans: Dict[tuple, VarPlan] = {}
_signal_plans: Dict[tuple, VarPlan] = {}
_smooth_plans: Dict[tuple, VarPlan] = {}      # edge_aware_smooth, forms "planes" and "power"


def _cached_plan(cache: Dict[tuple, VarPlan], create, shape, scans, planes: int, n_weights: int, device) -> VarPlan:
    """the plan of `cache` for these arguments, made by `create` (VarPlan, VarPlan.signal or VarPlan.volume) where there is none yet"""
    key = (shape, tuple((int(d), bool(c), int(k)) for d, c, k in scans), int(planes), int(n_weights), device)
    plan = cache.get(key)
    if plan is None:
        plan = cache[key] = create(key[0], key[1], planes=key[2], n_weights=key[3], device=device)
    return plan


def var_scan(ins, weights, scans):
    """`VarPlan.apply` without the plan: `scans` [(dim, causal, weight index), ...] on the device planes `ins` with the weight
    planes `weights`, differentiable with respect to both.  Plans are cached by shape, scans, plane counts and device; calls that
    share a plan are ordered by the caller (one stream)."""
    ins, weights = list(ins), list(weights)
    return _cached_plan(_scan_plans, VarPlan, tuple(ins[0].shape), scans, len(ins), len(weights), _device_index(ins[0])).apply(ins, weights)


def var_scan_volume(ins, weights, scans):
    """`scans` [(dim, causal, weight index), ...] with dim 0 = x, 1 = y, 2 = z on the device volumes `ins` (f32, one shape
    (D, H, W)) with the weight volumes `weights`, through a cached `VarPlan.volume`; differentiable with respect to both, like
    `var_scan`.  Element 0 of a weight volume along the scanned axis is never used.  Calls that share a plan are ordered by the
    caller (one stream).  Returns a tuple of len(ins) volumes."""
    import torch
    ins, weights = list(ins), list(weights)
    shape = tuple(int(s) for s in ins[0].shape)
    if len(shape) != 3 or any(tuple(t.shape) != shape for t in ins + weights):
        raise ValueError("var_scan_volume takes 3-D volumes (D, H, W) of one shape")
    plan = _cached_plan(_volume_plans, VarPlan.volume, shape, scans, len(ins), len(weights), _device_index(ins[0]))
    with torch.cuda.device(ins[0].device):
        return plan.apply(ins, weights)


def _padded(t, pad: int, value: float):
    """`pad` more elements of `value` behind a 1-D tensor (differentiable: the gradient is the slice)"""
    import torch
    return t if pad == 0 else torch.nn.functional.pad(t, (0, pad), value=value)


def var_scan_signal(ins, weights, scans):
    """`scans` [(0, causal, weight index), ...] on the 1-D device signals `ins` (f32, one length N) with the weight signals
    `weights`, through a cached `VarPlan.signal`; differentiable with respect to both, like `var_scan`.  Element 0 of a weight
    signal is never used.  The library takes lengths that are multiples of 4: any other length is padded up to the next one --
    the inputs with 0 and the weights with 0, and a weight of 0 decouples exactly, so the N real samples are what an unpadded
    scan gives -- and the result is sliced back.  The padding costs one copy of every signal (none where N % 4 == 0).  Calls that
    share a plan are ordered by the caller (one stream).  Returns a tuple of len(ins) signals."""
    import torch
    ins, weights = list(ins), list(weights)
    n = int(ins[0].shape[0])
    if any(t.dim() != 1 or int(t.shape[0]) != n for t in ins + weights):
        raise ValueError("var_scan_signal takes 1-D signals of one length")
    pad = -n % 4
    plan = _cached_plan(_signal_plans, VarPlan.signal, n + pad, scans, len(ins), len(weights), _device_index(ins[0]))
    with torch.cuda.device(ins[0].device):
        outs = plan.apply([_padded(t, pad, 0.0) for t in ins], [_padded(w, pad, 0.0) for w in weights])
    return tuple(o[:n] for o in outs) if pad else tuple(outs)


def smooth_samples(x, gaps, time_constant, zero_phase: bool = True):
    """The exponential moving average of an irregularly sampled series: x (N,) or (C, N), f32 on the device, sampled at times t
    with gaps[i] = t[i] - t[i-1] >= 0 (gaps[0] is unused):
        y[i] = (1 - w[i]) x[i] + w[i] y[i-1],   w[i] = exp(-gaps[i] / time_constant)
    and, with zero_phase, the same recurrence backwards over the result (+x -x, one fused stage).  It runs through the power form
    of a cached `VarPlan.signal`: the weights are formed in the kernels as base ** gaps with base = exp(-1 / time_constant), and no
    weight signal is stored.  Differentiable with respect to x and gaps -- and with respect to the time constant where that is a
    float tensor of one element (dL/dtau = dL/dbase * base / tau^2, dL/dbase from `VarPlan.backward_power_bases`; reading its value
    costs one host read per call).  A time constant whose base rounds to 0 or 1 in f32 is
    refused by the library (RecFilterError).  Lengths that are not multiples of 4 are padded as in `var_scan_signal` (the gaps with
    +inf: a weight of exactly 0), at the cost of one copy."""
    import torch
    if x.dim() not in (1, 2) or gaps.dim() != 1 or int(gaps.shape[0]) != int(x.shape[-1]):
        raise ValueError(f"x must be (N,) or (C, N) and gaps (N,), got {tuple(x.shape)} and {tuple(gaps.shape)}")
    signals = [x] if x.dim() == 1 else [x[c] for c in range(x.shape[0])]
    n = int(gaps.shape[0])
    pad = -n % 4
    if isinstance(time_constant, torch.Tensor):
        if not time_constant.is_floating_point() or time_constant.numel() != 1:
            raise ValueError("a tensor time_constant must be a float tensor of one element")
        base = torch.exp(-1.0 / time_constant.reshape(1).to(torch.float64))      # (autograd: d base / d tau = base / tau^2)
    else:
        base = [math.exp(-1.0 / float(time_constant))]
    scans = [(0, True, 0), (0, False, 0)] if zero_phase else [(0, True, 0)]
    plan = _cached_plan(_signal_plans, VarPlan.signal, n + pad, scans, len(signals), 1, _device_index(x))
    with torch.cuda.device(x.device):
        outs = plan.apply_power([_padded(t.to(torch.float32), pad, 0.0) for t in signals], [_padded(gaps.to(torch.float32), pad, math.inf)], base)
    outs = [o[:n] for o in outs] if pad else list(outs)
    return outs[0] if x.dim() == 1 else torch.stack(outs)


# ---- the domain-transform recursive filter ----------------------------------------------------------------------------------
def domain_transform_weights(guide, sigma_s: float, sigma_r: float, iterations: int = 3):
    """The feedback planes of the domain-transform recursive filter for a guide image (C, H, W) or (H, W), computed with torch on
    the guide's device:  [(w_x, w_y) for iteration k = 0 .. iterations-1],  f32 planes of (H, W) with
        d_x[i] = 1 + (sigma_s / sigma_r) * sum_c |g_c[i] - g_c[i-1]|     (the same along y; element 0, never used, holds a^1)
        sigma_k = sigma_s * sqrt(3) * 2^(K-1-k) / sqrt(4^K - 1),   a_k = exp(-sqrt(2) / sigma_k),   w = a_k ** d."""
    import torch
    if iterations < 1:
        raise ValueError("iterations must be >= 1")
    g = guide if guide.dim() == 3 else guide.unsqueeze(0)
    if g.dim() != 3:
        raise ValueError(f"guide must be (C, H, W) or (H, W), got {tuple(guide.shape)}")
    g = g.to(torch.float32)
    ratio = float(sigma_s) / float(sigma_r)
    dx = torch.ones(g.shape[1:], dtype=torch.float32, device=g.device)
    dy = torch.ones(g.shape[1:], dtype=torch.float32, device=g.device)
    dx[:, 1:] += ratio * (g[:, :, 1:] - g[:, :, :-1]).abs().sum(0)
    dy[1:, :] += ratio * (g[:, 1:, :] - g[:, :-1, :]).abs().sum(0)
    return [(torch.pow(a_k, dx).contiguous(), torch.pow(a_k, dy).contiguous()) for a_k in domain_transform_bases(sigma_s, iterations)]


def domain_transform_bases(sigma_s: float, iterations: int = 3) -> List[float]:
    """[a_0 .. a_{K-1}] of the domain-transform recursive filter:
        sigma_k = sigma_s * sqrt(3) * 2^(K-1-k) / sqrt(4^K - 1),   a_k = exp(-sqrt(2) / sigma_k)."""
    if iterations < 1:
        raise ValueError("iterations must be >= 1")
    K = int(iterations)
    out = []
    for k in range(K):
        sigma_k = float(sigma_s) * math.sqrt(3.0) * 2.0 ** (K - 1 - k) / math.sqrt(4.0 ** K - 1.0)
        out.append(math.exp(-math.sqrt(2.0) / sigma_k))
    return out


def _distance_guide(guide, nd: int, sigma_s: float, sigma_r: float, backward: bool = False):
    """(the guide with its channel axis, contiguous; its planes' pointer array; the scale) for the distance calls on `nd` spatial
    dimensions, after the checks they share; backward: f32 guides only"""
    import torch
    g = guide if guide.dim() == nd + 1 else guide.unsqueeze(0)
    if g.dim() != nd + 1:
        raise ValueError(f"guide must be {'(C, H, W) or (H, W)' if nd == 2 else '(C, D, H, W) or (D, H, W)'}, got {tuple(guide.shape)}")
    if backward and g.dtype != torch.float32:
        raise TypeError(f"float32 guides only (there is no gradient with respect to a byte guide), got {g.dtype}")
    if g.dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"float32 or uint8 guides only, got {g.dtype}")
    if not g.is_cuda:
        raise ValueError("the guide must be a device tensor")
    g = g.contiguous()
    scale = float(sigma_s) / float(sigma_r) / (255.0 if g.dtype == torch.uint8 else 1.0)
    return g, (ctypes.c_void_p * g.shape[0])(*[g[c].data_ptr() for c in range(g.shape[0])]), scale


def _distance_gradients(g, grads, grad_guide, accumulate: bool):
    """(grad_guide, allocated where it is None; its planes' pointer array) for the distance adjoints of the guide `g`, after the
    checks of the gradient tensors: `grads` are those of d_x, d_y(, d_z)"""
    import torch
    if grad_guide is None:
        if accumulate:
            raise ValueError("accumulate=True needs grad_guide")
        grad_guide = torch.empty_like(g)
    gg = grad_guide if grad_guide.dim() == g.dim() else grad_guide.unsqueeze(0)
    shape = tuple(int(s) for s in g.shape)
    for what, t, want in [(f"grad_d{axis}", t, shape[1:]) for axis, t in zip("xyz", grads)] + [("grad_guide", gg, shape)]:
        if tuple(t.shape) != want or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float32 device tensor of shape {want}")
    return grad_guide, (ctypes.c_void_p * shape[0])(*[gg[c].data_ptr() for c in range(shape[0])])


def domain_transform_distances(guide, sigma_s: float, sigma_r: float, stream=None):
    """(d_x, d_y): the exponent planes of the domain-transform filter for a device guide image (C, H, W) or (H, W), f32 or uint8,
    by rf_var_distances (one HIP launch, one read of the guide):
        d_x[r][c] = 1 + scale * sum_ch |g_ch[r][c] - g_ch[r][c-1]|     (the same along y; column 0 of d_x and row 0 of d_y hold 1)
    scale = sigma_s / sigma_r, for a uint8 guide sigma_s / sigma_r / 255: a byte guide means that guide divided by 255.
    W must be a multiple of 4.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    g, planes, scale = _distance_guide(guide, 2, sigma_s, sigma_r)
    C, H, W = (int(s) for s in g.shape)
    dx, dy = (torch.empty((H, W), dtype=torch.float32, device=g.device) for _ in range(2))
    with torch.cuda.device(g.device):
        capi.check(capi.lib().rf_var_distances(planes, C, int(g.dtype == torch.uint8), W, H, scale, dx.data_ptr(), dy.data_ptr(), g.device.index,
                                               VarPlan._stream(stream)))
    return dx, dy


def domain_transform_distances_volume(guide, sigma_s: float, sigma_r: float, spacing_z: float = 1.0, stream=None):
    """(d_x, d_y, d_z): the exponent volumes of the domain-transform filter for a device guide volume (C, D, H, W) or (D, H, W),
    f32 or uint8, by rf_var_distances_volume (one HIP launch, one read of the guide).  d_x and d_y are, slice by slice, what
    `domain_transform_distances` gives;
        d_z[z][r][c] = spacing_z + scale * sum_ch |g_ch[z][r][c] - g_ch[z-1][r][c]|     (slice 0 holds spacing_z)
    with scale as there.  spacing_z > 0 is the sample distance along z in units of the x/y pitch (slice thickness, or how far
    apart two frames count); 1 = isotropic.  W must be a multiple of 4.  Asynchronous on `stream`."""
    import torch
    g, volumes, scale = _distance_guide(guide, 3, sigma_s, sigma_r)
    C, D, H, W = (int(s) for s in g.shape)
    dx, dy, dz = (torch.empty((D, H, W), dtype=torch.float32, device=g.device) for _ in range(3))
    with torch.cuda.device(g.device):
        capi.check(capi.lib().rf_var_distances_volume(volumes, C, int(g.dtype == torch.uint8), W, H, D, scale, float(spacing_z), dx.data_ptr(),
                                                      dy.data_ptr(), dz.data_ptr(), g.device.index, VarPlan._stream(stream)))
    return dx, dy, dz


def domain_transform_distances_backward(guide, sigma_s: float, sigma_r: float, grad_dx, grad_dy, grad_guide=None, accumulate: bool = False,
                                        stream=None):
    """rf_var_distances_backward: the gradient of an f32 device guide (C, H, W) or (H, W) from the gradients of the two planes of
    `domain_transform_distances` (one HIP launch, a gather).  grad_guide=None allocates it (then accumulate must be False);
    accumulate=True adds to what grad_guide holds.  Returned in the guide's shape."""
    import torch
    g, planes, scale = _distance_guide(guide, 2, sigma_s, sigma_r, backward=True)
    C, H, W = (int(s) for s in g.shape)
    grad_guide, grads = _distance_gradients(g, (grad_dx, grad_dy), grad_guide, accumulate)
    with torch.cuda.device(g.device):
        capi.check(capi.lib().rf_var_distances_backward(planes, C, W, H, scale, grad_dx.data_ptr(), grad_dy.data_ptr(), grads,
                                                        int(bool(accumulate)), g.device.index, VarPlan._stream(stream)))
    return grad_guide


def domain_transform_distances_volume_backward(guide, sigma_s: float, sigma_r: float, grad_dx, grad_dy, grad_dz, grad_guide=None,
                                               accumulate: bool = False, stream=None):
    """rf_var_distances_volume_backward: the gradient of an f32 device guide volume (C, D, H, W) or (D, H, W) from the gradients of
    the three volumes of `domain_transform_distances_volume` (one HIP launch, var_distances_volume_grad, a gather; spacing_z does
    not enter).  grad_guide=None allocates it (then accumulate must be False); accumulate=True adds to what grad_guide holds.
    Returned in the guide's shape."""
    import torch
    g, volumes, scale = _distance_guide(guide, 3, sigma_s, sigma_r, backward=True)
    C, D, H, W = (int(s) for s in g.shape)
    grad_guide, grads = _distance_gradients(g, (grad_dx, grad_dy, grad_dz), grad_guide, accumulate)
    with torch.cuda.device(g.device):
        capi.check(capi.lib().rf_var_distances_volume_backward(volumes, C, W, H, D, scale, grad_dx.data_ptr(), grad_dy.data_ptr(),
                                                               grad_dz.data_ptr(), grads, int(bool(accumulate)), g.device.index,
                                                               VarPlan._stream(stream)))
    return grad_guide


class SmoothPlan(_PlanHandle):
    """rf_smooth_plan_*: the domain-transform recursive filter of `planes` image planes of `shape_hw` = (height, width), f32 or
    uint8 (uint8: input AND output; out = sat8 of the f32 filter on the widened bytes, rounded once, at the final store).
    guide_planes = 0: the image guides itself; else that many separate guide planes of `guide_dtype`.  A byte guide means that
    guide divided by 255.  One var_distances launch, then 6 launches per iteration.  One plan owns its distance planes, working
    planes, tails and carries: order its executes.
    batch=N (rf_smooth_plan_create_batched): N images per call, every launch taking all of them -- the launch counts are those of
    one image.  Image, output and gradient tensors are then contiguous (N, planes, H, W) device tensors and the guide
    (N, guide_planes, H, W); every image is filtered with its own edges, bit for bit as a plan without a batch filters it.
    batch=None: one image, through rf_smooth_plan_create."""
    _destroy = "rf_smooth_plan_destroy"

    def __init__(self, shape_hw: Sequence[int], planes: int = 1, guide_planes: int = 0, image_dtype=None, guide_dtype=None,
                 iterations: int = 3, sigma_s: float = 60.0, sigma_r: float = 0.4, device: int = -1, batch: Optional[int] = None):
        shape_hw = tuple(int(s) for s in shape_hw)
        if len(shape_hw) != 2:
            raise ValueError(f"shape_hw must be (height, width), got {shape_hw}")
        d = self._describe(capi.SmoothDesc(), shape_hw, planes, guide_planes, image_dtype, guide_dtype, iterations, sigma_s, sigma_r, device)
        d.height, d.width = shape_hw
        self.batch = None if batch is None else int(batch)
        if self.batch is None:
            capi.check(capi.lib().rf_smooth_plan_create(ctypes.byref(d), ctypes.byref(self._h)))
        else:
            b = capi.SmoothBatchDesc()      # contiguous NCHW
            b.batch = self.batch
            b.image_stride = d.n_planes * d.height * d.width
            b.guide_stride = d.n_guide * d.height * d.width
            capi.check(capi.lib().rf_smooth_plan_create_batched(ctypes.byref(d), ctypes.byref(b), ctypes.byref(self._h)))

    def _describe(self, d, shape, planes, guide_planes, image_dtype, guide_dtype, iterations, sigma_s, sigma_r, device):
        """what an image plan and a volume plan share: the dtype checks, the common fields of the description `d` (flags 0, no
        extents) and the attributes (batch None, no handle yet); returns d"""
        import torch
        image_dtype = torch.float32 if image_dtype is None else image_dtype
        guide_dtype = torch.float32 if guide_dtype is None else guide_dtype
        for what, dt in (("image", image_dtype), ("guide", guide_dtype)):
            if dt not in (torch.float32, torch.uint8):
                raise TypeError(f"{what}_dtype must be torch.float32 or torch.uint8, got {dt}")
        d.abi = capi.RF_ABI
        d.image_u8 = int(image_dtype == torch.uint8)
        d.n_planes, d.n_guide = int(planes), int(guide_planes)
        d.guide_u8 = int(guide_dtype == torch.uint8) if d.n_guide != 0 else 0
        d.iterations = int(iterations)
        d.sigma_s, d.sigma_r = float(sigma_s), float(sigma_r)
        d.device = int(device)
        d.flags = 0
        self._desc = d
        self.shape, self.planes, self.guide_planes, self.iterations = shape, int(planes), int(guide_planes), int(iterations)
        self.image_dtype, self.guide_dtype = image_dtype, guide_dtype if d.n_guide != 0 else None
        self.batch = None
        self._h = ctypes.c_void_p()
        return d

    @classmethod
    def volume(cls, shape_dhw: Sequence[int], planes: int = 1, guide_planes: int = 0, image_dtype=None, guide_dtype=None,
               iterations: int = 3, sigma_s: float = 60.0, sigma_r: float = 0.4, spacing_z: float = 1.0, device: int = -1,
               differentiable: bool = False) -> "SmoothPlan":
        """rf_smooth_plan_create_volume: the filter along x, y and z of `planes` volumes of `shape_dhw` = (depth, height, width),
        f32 or uint8 (bytes in, bytes out, as for images).  The plan owns three distance volumes: one var_distances_volume
        launch, then 9 launches per iteration (+x -x, +y -y, +z -z).  spacing_z > 0: the sample distance along z in units of the
        x/y pitch.  execute / execute_timed take (C, D, H, W) or (D, H, W) tensors (or lists of (D, H, W) volumes); there is no
        batch of volumes.
        differentiable=False: backward is refused by the library (RF_ERR_UNSUPPORTED) and its queries return 0.
        differentiable=True (RF_SMOOTH_VOLUME_BACKWARD; f32 volumes, the library refuses uint8 ones at create): the same forward,
        bit for bit, and `backward`, `backward_timed` and `apply` work as on an image plan -- 1 + 18 K launches with the
        distances held constant, 51 K - 7 through them (the last one var_distances_volume_grad), and
        3 + (K - 1 + 7) * planes f32 volumes of workspace allocated by the first edges=True call."""
        self = cls.__new__(cls)
        shape_dhw = tuple(int(s) for s in shape_dhw)
        if len(shape_dhw) != 3:
            raise ValueError(f"shape_dhw must be (depth, height, width), got {shape_dhw}")
        d = self._describe(capi.SmoothVolumeDesc(), shape_dhw, planes, guide_planes, image_dtype, guide_dtype, iterations, sigma_s, sigma_r, device)
        d.depth, d.height, d.width = shape_dhw
        d.spacing_z = float(spacing_z)
        d.flags = capi.RF_SMOOTH_VOLUME_BACKWARD if differentiable else 0
        capi.check(capi.lib().rf_smooth_plan_create_volume(ctypes.byref(d), ctypes.byref(self._h)))
        return self

    # -- queries ----------------------------------------------------------------------------
    @property
    def workspace_bytes(self) -> int:
        return int(capi.lib().rf_smooth_plan_workspace_bytes(self._h))

    @property
    def num_kernels(self) -> int:
        return int(capi.lib().rf_smooth_plan_num_kernels(self._h))

    @property
    def bases(self) -> List[float]:
        """[a_0 .. a_{K-1}]: the f32 bases the plan runs with"""
        out = (ctypes.c_float * self.iterations)()
        capi.check(capi.lib().rf_smooth_plan_bases(self._h, out))
        return [float(v) for v in out]

    def set_sigmas(self, sigma_s: float, sigma_r: float) -> None:
        """rf_smooth_plan_set_sigmas: new sigmas for this plan -- the scale of the distances and the bases are recomputed as create
        computes them (`bases` afterwards is a fresh plan's, bit for bit), nothing is allocated, and every later execute and
        backward runs with them.  Refused like create's sigmas, the plan left unchanged.  Works on host-only plans.  Order it
        against the plan's executes as an execute is ordered."""
        capi.check(capi.lib().rf_smooth_plan_set_sigmas(self._h, float(sigma_s), float(sigma_r)))
        self._desc.sigma_s, self._desc.sigma_r = float(sigma_s), float(sigma_r)

    # -- execution --------------------------------------------------------------------------
    def _pointers(self, tensor, count: int, dtype, what: str) -> ctypes.Array:
        """the planes of a (C, H, W) or (H, W) device tensor, or of a list of (H, W) tensors; VarPlan._pointers' checks.
        A batched plan: image 0's planes of a contiguous (N, C, H, W) device tensor (the plan holds the strides)."""
        if self.batch is not None:
            shape = (self.batch, count) + self.shape
            if not hasattr(tensor, "dim") or tensor.dim() != 4:
                raise ValueError(f"{what} must be one (N, C, H, W) tensor for a batched plan")
            if tuple(tensor.shape) != shape:
                raise ValueError(f"{what}: shape {tuple(tensor.shape)} != the batched plan's {shape}")
            if tensor.dtype != dtype:
                raise TypeError(f"{what}: {dtype} planes only, got {tensor.dtype}")
            if not tensor.is_cuda or not tensor.is_contiguous():
                raise ValueError(f"{what} must be a contiguous device tensor")
            return (ctypes.c_void_p * count)(*[tensor[0, c].data_ptr() for c in range(count)])
        if hasattr(tensor, "dim"):
            nd = len(self.shape)      # 2, or 3 for a volume plan: one plane, or a stack of planes
            tensor = [tensor] if tensor.dim() == nd else [tensor[c] for c in range(tensor.shape[0])] if tensor.dim() == nd + 1 else None
            if tensor is None:
                raise ValueError(f"{what} must be (C, H, W) or (H, W)" if nd == 2 else f"{what} must be (C, D, H, W) or (D, H, W)")
        if len(tensor) != count:
            raise ValueError(f"expected {count} {what} planes, got {len(tensor)}")
        arr = (ctypes.c_void_p * count)()
        for i, t in enumerate(tensor):
            arr[i] = _plane_pointer(t, self.shape, dtype, str(dtype), f"{what} plane {i}")
        return arr

    def _arguments(self, image, guide, out, stream):
        """(image, guide and output pointers, the output, the stream's handle)"""
        import torch
        nulls = _host_only_nulls(self, self.planes, self.guide_planes or None, self.planes)
        if nulls:
            return (*nulls, None, ctypes.c_void_p())
        if out is None:
            out = torch.empty_like(image) if hasattr(image, "dim") else [torch.empty_like(t) for t in image]
        pg = None
        if guide is not None:
            if self.guide_planes == 0:
                raise ValueError("this plan's image guides itself (guide_planes=0): no guide is taken")
            pg = self._pointers(guide, self.guide_planes, self.guide_dtype, "guide")
        elif self.guide_planes != 0:
            raise ValueError(f"this plan takes {self.guide_planes} separate guide planes")
        return self._pointers(image, self.planes, self.image_dtype, "image"), pg, self._pointers(out, self.planes, self.image_dtype, "output"), out, self._stream(stream)

    def execute(self, image, guide=None, out=None, stream=None):
        """rf_smooth_plan_execute: asynchronous on `stream` (default: torch's current stream).  image, out: (C, H, W) or (H, W)
        device tensors of the plan's image dtype (or lists of (H, W) planes); out=None allocates it; out may be the image."""
        pi, pg, po, out, s = self._arguments(image, guide, out, stream)
        capi.check(capi.lib().rf_smooth_plan_execute(self._h, pi, pg, po, s))
        return out

    def execute_timed(self, image, guide=None, out=None, stream=None):
        """rf_smooth_plan_execute_timed: (output, [(kernel name, ms), ...]) measured with HIP events; synchronises the stream."""
        pi, pg, po, out, s = self._arguments(image, guide, out, stream)
        return out, _timed(lambda *report: capi.lib().rf_smooth_plan_execute_timed(self._h, pi, pg, po, s, *report), self.num_kernels)

    # -- the adjoint ------------------------------------------------------------------------
    def backward_num_kernels(self, edges: bool = False) -> int:
        """rf_smooth_plan_backward_num_kernels: 1 + 12 K launches with the distances held constant, 34 K - 4 through them (a
        differentiable volume plan: 1 + 18 K and 51 K - 7; a volume plan without the flag: 0)"""
        return int(capi.lib().rf_smooth_plan_backward_num_kernels(self._h, int(bool(edges))))

    def backward_workspace_bytes(self, edges: bool = False) -> int:
        """rf_smooth_plan_backward_workspace_bytes: what the first backward call with edges allocates beyond workspace_bytes,
        2 + (K - 1 + 5) * planes f32 planes (a differentiable volume plan: 3 + (K - 1 + 7) * planes f32 volumes); 0 without edges"""
        return int(capi.lib().rf_smooth_plan_backward_workspace_bytes(self._h, int(bool(edges))))

    def _backward_arguments(self, image, guide, grad_out, grad_image, grad_guide, edges, stream):
        """(the five pointer arrays, grad_image, grad_guide, the stream's handle)"""
        import torch
        nulls = _host_only_nulls(self, self.planes if image is not None else None, self.guide_planes if guide is not None else None, self.planes,
                                 self.planes, self.guide_planes if grad_guide is not None else None)
        if nulls:
            return (*nulls, None, None, ctypes.c_void_p())
        f32 = torch.float32
        if grad_image is None:
            grad_image = torch.empty_like(grad_out) if hasattr(grad_out, "dim") else [torch.empty_like(t) for t in grad_out]
        if edges and self.guide_planes and grad_guide is None and guide is not None and self.guide_dtype == f32:
            grad_guide = torch.empty_like(guide) if hasattr(guide, "dim") else [torch.empty_like(t) for t in guide]
        return (self._pointers(image, self.planes, f32, "image") if image is not None else None,
                self._pointers(guide, self.guide_planes, self.guide_dtype, "guide") if guide is not None else None,
                self._pointers(grad_out, self.planes, f32, "grad_out"), self._pointers(grad_image, self.planes, f32, "grad_image"),
                self._pointers(grad_guide, self.guide_planes, f32, "grad_guide") if grad_guide is not None else None,
                grad_image, grad_guide, self._stream(stream))

    def backward(self, image, guide, grad_out, grad_image=None, grad_guide=None, edges: bool = False, stream=None):
        """rf_smooth_plan_backward, the adjoint of execute for f32 images: (grad_image, grad_guide) from grad_out = dL/d(out).
        edges=False holds the distances constant (grad_guide is None; `image` is needed only where the image guides itself).
        edges=True differentiates through them: with separate f32 guide planes grad_guide is written (allocated when None); where
        the image guides itself that gradient is added into grad_image.  grad_image=None allocates it; it may be grad_out (in
        place).  Asynchronous on `stream`; uses the plan's workspace like an execute."""
        pi, pg, pgo, pgi, pgg, grad_image, grad_guide, s = self._backward_arguments(image, guide, grad_out, grad_image, grad_guide, edges, stream)
        capi.check(capi.lib().rf_smooth_plan_backward(self._h, pi, pg, pgo, pgi, pgg, int(edges), s))
        return grad_image, grad_guide

    def backward_timed(self, image, guide, grad_out, grad_image=None, grad_guide=None, edges: bool = False, stream=None):
        """rf_smooth_plan_backward_timed: (grad_image, grad_guide, [(kernel name, ms), ...]); synchronises the stream"""
        pi, pg, pgo, pgi, pgg, grad_image, grad_guide, s = self._backward_arguments(image, guide, grad_out, grad_image, grad_guide, edges, stream)
        return grad_image, grad_guide, _timed(lambda *report: capi.lib().rf_smooth_plan_backward_timed(self._h, pi, pg, pgo, pgi, pgg, int(edges), s, *report),
                                              self.backward_num_kernels(edges))

    def backward_sigmas_num_kernels(self, edges: bool = False) -> int:
        """rf_smooth_plan_backward_sigmas_num_kernels: backward_num_kernels(True), less the distances' adjoint without edges, and two"""
        return int(capi.lib().rf_smooth_plan_backward_sigmas_num_kernels(self._h, int(bool(edges))))

    def _grad_params(self, grad_params, like):
        import torch
        if self._desc.device == capi.RF_DEVICE_HOST_ONLY:
            return None, ctypes.c_void_p()
        n = 3 + self.iterations
        if grad_params is None:
            grad_params = torch.empty(n, dtype=torch.float64, device=like.device)
        if grad_params.dtype != torch.float64 or tuple(grad_params.shape) != (n,) or not grad_params.is_cuda or not grad_params.is_contiguous():
            raise ValueError(f"grad_params must be a contiguous float64 device tensor of {n} entries")
        return grad_params, ctypes.c_void_p(grad_params.data_ptr())

    def backward_sigmas(self, image, guide, grad_out, grad_image=None, grad_guide=None, edges: bool = False, grad_params=None, stream=None):
        """rf_smooth_plan_backward_sigmas: (grad_image, grad_guide, grad_params).  `backward` with the same `edges` -- grad_image and
        grad_guide are its bits -- and grad_params, a float64 DEVICE tensor of 3 + iterations entries (None allocates it):
        dL/dsigma_s, dL/dsigma_r, dL/dspacing_z (0 on an image plan), dL/da_0 .. dL/da_{K-1}, summed over the batch.  `image` is
        always needed; a uint8 guide is allowed without edges.  Asynchronous: reading grad_params on the host synchronises."""
        pi, pg, pgo, pgi, pgg, grad_image, grad_guide, s = self._backward_arguments(image, guide, grad_out, grad_image, grad_guide, edges, stream)
        grad_params, pgp = self._grad_params(grad_params, grad_image if hasattr(grad_image, "device") else (grad_image[0] if grad_image else None))
        capi.check(capi.lib().rf_smooth_plan_backward_sigmas(self._h, pi, pg, pgo, pgi, pgg, int(edges), pgp, s))
        return grad_image, grad_guide, grad_params

    def backward_sigmas_timed(self, image, guide, grad_out, grad_image=None, grad_guide=None, edges: bool = False, grad_params=None, stream=None):
        """rf_smooth_plan_backward_sigmas_timed: (grad_image, grad_guide, grad_params, [(kernel name, ms), ...])"""
        pi, pg, pgo, pgi, pgg, grad_image, grad_guide, s = self._backward_arguments(image, guide, grad_out, grad_image, grad_guide, edges, stream)
        grad_params, pgp = self._grad_params(grad_params, grad_image if hasattr(grad_image, "device") else (grad_image[0] if grad_image else None))
        timings = _timed(lambda *report: capi.lib().rf_smooth_plan_backward_sigmas_timed(self._h, pi, pg, pgo, pgi, pgg, int(edges), pgp, s, *report),
                         self.backward_sigmas_num_kernels(edges))
        return grad_image, grad_guide, grad_params, timings

    def apply(self, image, guide=None, sigma_s=None, sigma_r=None):
        """execute, out of place, as a differentiable torch operation on f32 tensors (C, H, W) or (H, W) -- on a volume plan made
        with differentiable=True, (C, D, H, W) or (D, H, W): values bit for bit execute's.  Backward is `backward`; it goes through the distances (edges) where the guide requires a gradient, or the
        image does and guides itself.  Only the image and the guide are saved; no double backward.
        sigma_s, sigma_r: None (the plan's sigmas, constants) -- or both given, floats or float tensors of one element: the
        plan is given these sigmas (`set_sigmas`) before the forward AND again before the backward, so calls with different
        sigmas may share one plan, and a tensor that requires a gradient receives one (backward is then `backward_sigmas`).
        Reading a sigma tensor costs one host read per call."""
        if (sigma_s is None) != (sigma_r is None):
            raise ValueError("sigma_s and sigma_r: both or neither")
        if sigma_s is None:
            return _smooth_function().apply(self, image, guide)
        return _smooth_function().apply(self, image, guide, sigma_s, sigma_r)


_smooth_fn = None


def _smooth_function():
    """the torch.autograd.Function behind SmoothPlan.apply (torch is imported when it is first needed)"""
    global _smooth_fn
    if _smooth_fn is not None:
        return _smooth_fn
    import torch
    planes = _aligned_contiguous

    def scalar(v):
        """(the value, what a gradient for it looks like or None) of a sigma given as a float or as a tensor of one element"""
        if isinstance(v, torch.Tensor):
            if not v.is_floating_point() or v.numel() != 1:
                raise ValueError("a tensor sigma must be a float tensor of one element")
            return float(v.detach().to(torch.float64).cpu().item()), (v.shape, v.dtype, v.device)      # (the one host read)
        return float(v), None

    class SmoothFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, image, guide, sigma_s=None, sigma_r=None):
            image = planes(image)
            guide = planes(guide) if guide is not None else None
            ctx.plan = plan
            ctx.sigmas = None
            if sigma_s is not None:
                (vs, like_s), (vr, like_r) = scalar(sigma_s), scalar(sigma_r)
                ctx.sigmas = (vs, vr, like_s, like_r)
                plan.set_sigmas(vs, vr)
            ctx.save_for_backward(image, *([guide] if guide is not None else []))
            with torch.cuda.device(image.device):
                return plan.execute(image, guide)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            plan = ctx.plan
            image = ctx.saved_tensors[0]
            guide = ctx.saved_tensors[1] if len(ctx.saved_tensors) > 1 else None
            need_image, need_guide = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
            edges = need_guide if guide is not None else need_image
            if ctx.sigmas is None:
                with torch.cuda.device(image.device):
                    grad_image, grad_guide = plan.backward(image, guide, planes(grad_out), None, None, edges=bool(edges))
                return None, grad_image if need_image else None, grad_guide if need_guide else None
            vs, vr, like_s, like_r = ctx.sigmas
            need_s, need_r = like_s is not None and ctx.needs_input_grad[3], like_r is not None and ctx.needs_input_grad[4]
            plan.set_sigmas(vs, vr)      # (another call may have given the shared plan other sigmas since the forward)
            with torch.cuda.device(image.device):
                if need_s or need_r:
                    grad_image, grad_guide, gp = plan.backward_sigmas(image, guide, planes(grad_out), None, None, edges=bool(edges))
                else:
                    grad_image, grad_guide = plan.backward(image, guide, planes(grad_out), None, None, edges=bool(edges))
            like = lambda g, l: g.to(device=l[2], dtype=l[1]).reshape(l[0])      # noqa: E731
            return (None, grad_image if need_image else None, grad_guide if need_guide else None,
                    like(gp[0], like_s) if need_s else None, like(gp[1], like_r) if need_r else None)

    _smooth_fn = SmoothFunction
    return _smooth_fn


_smooth_plan_objects: Dict[tuple, SmoothPlan] = {}      # form="plan": keyed by shape, dtypes, iterations, sigmas and device
_smooth_volume_plans: Dict[tuple, SmoothPlan] = {}      # the same with spacing_z, and whether the plan has a backward


def _smooth_by_plan(image, guide, sigma_s, sigma_r, iterations, differentiable=False, nd: int = 2, spacing_z: float = 1.0):
    """form="plan" (nd = 2): one cached SmoothPlan on (C, H, W) or (H, W), on (N, C, H, W) one cached SmoothPlan(batch=N) by the same
    rules; and edge_aware_smooth_volume (nd = 3): one cached SmoothPlan.volume on (C, D, H, W) or (D, H, W), which has no batch"""
    import torch
    what, dims, guide_dims, extents = (("image", "(C, H, W) or (H, W)", "(C, H, W) or (H, W)", "height and width") if nd == 2 else
                                       ("volume", "(C, D, H, W) or (D, H, W)", "(G, D, H, W) or (D, H, W)", "depth, height and width"))
    batched = nd == 2 and image.dim() == 4
    at = 1 if batched else 0      # where the planes are counted
    img = image if batched or image.dim() == nd + 1 else image.unsqueeze(0)
    if img.dim() != nd + 1 + at:
        raise ValueError(f"{what} must be {dims}, got {tuple(image.shape)}")
    if img.dtype != torch.uint8:
        img = img.to(torch.float32)
    img = img.contiguous()
    g = None
    if guide is not None:
        if batched and guide.dim() != 4:
            raise ValueError(f"a batched image (N, C, H, W) takes a guide (N, G, H, W), got {tuple(guide.shape)}")
        g = guide if batched or guide.dim() == nd + 1 else guide.unsqueeze(0)
        if g.dim() != nd + 1 + at:
            raise ValueError(f"guide must be {guide_dims}, got {tuple(guide.shape)}")
        if g.dtype != torch.uint8:
            g = g.to(torch.float32)
        g = g.to(img.device).contiguous()
        if tuple(g.shape[:at]) != tuple(img.shape[:at]) or tuple(g.shape[at + 1:]) != tuple(img.shape[at + 1:]):
            raise ValueError(f"guide and {what} must have the same " + ("batch size, " if batched else "") + extents)
    shape = tuple(int(s) for s in img.shape)      # (C, H, W), (N, C, H, W) or (C, D, H, W)
    device = _device_index(img)
    tensor_sigmas = isinstance(sigma_s, torch.Tensor) or isinstance(sigma_r, torch.Tensor)
    if tensor_sigmas and not differentiable:
        raise TypeError("tensor sigmas are taken with differentiable=True")
    wants_grad = bool(differentiable) and torch.is_grad_enabled() and (img.requires_grad or (g is not None and g.requires_grad) or
                                                                      any(isinstance(v, torch.Tensor) and v.requires_grad for v in (sigma_s, sigma_r)))
    if wants_grad and (img.dtype != torch.float32 or (g is not None and g.dtype != torch.float32 and g.requires_grad)):
        raise TypeError("differentiable=True takes f32 images, and f32 guides where the guide requires a gradient")
    n_guide = 0 if g is None else int(g.shape[at])
    # tensor sigmas: one plan for every value (the key leaves them out; SmoothPlan.apply sets them before forward and backward), at
    # the cost of one host read per sigma tensor and call
    first_s, first_r = (float(v.detach().cpu()) if isinstance(v, torch.Tensor) else float(v) for v in (sigma_s, sigma_r))
    common = dict(planes=shape[at], guide_planes=n_guide, image_dtype=img.dtype, guide_dtype=None if g is None else g.dtype, iterations=iterations,
                  sigma_s=first_s, sigma_r=first_r, device=device)
    key = shape + (img.dtype, None if g is None else (n_guide, g.dtype), int(iterations)) + (("tensor sigmas",) if tensor_sigmas else (first_s, first_r))
    if nd == 2:
        cache, key = _smooth_plan_objects, key + (device,)
    else:      # (a plan with a backward is built only where one is needed: the default call keeps the plans it had)
        cache, key = _smooth_volume_plans, key + (float(spacing_z), device, wants_grad)
    plan = cache.get(key)
    if plan is None and nd == 2:
        plan = cache[key] = SmoothPlan(shape[-2:], batch=shape[0] if batched else None, **common)
    elif plan is None:
        plan = cache[key] = SmoothPlan.volume(shape[1:], spacing_z=spacing_z, differentiable=wants_grad, **common)
    if tensor_sigmas:
        if img.dtype != torch.float32:
            raise TypeError("tensor sigmas take f32 images")
        out = plan.apply(img, g, sigma_s, sigma_r)      # (also without a gradient: the shared plan needs this call's sigmas)
    elif wants_grad:
        out = plan.apply(img, g)
    else:
        with torch.cuda.device(img.device):
            out = plan.execute(img, g)
    return out if image.dim() >= nd + 1 else out[0]


def edge_aware_smooth_volume(volume, guide=None, sigma_s: float = 60.0, sigma_r: float = 0.4, iterations: int = 3, spacing_z: float = 1.0,
                             differentiable: bool = False):
    """Edge-aware smoothing of a device volume (C, D, H, W) or (D, H, W), f32 or uint8, by the domain-transform recursive filter
    along x, y and z, through a cached `SmoothPlan.volume` (keyed by shape, dtypes, iterations, sigmas, spacing_z and device): per
    iteration +x -x, +y -y, +z -z on the three exponent volumes of `domain_transform_distances_volume`.  guide=None: the volume
    guides itself; else a guide (G, D, H, W) or (D, H, W), f32 or uint8.  spacing_z > 0 is the sample distance along z in units
    of the x/y pitch -- slice thickness of a CT/MR stack, or how far apart two video frames count; 1 = isotropic.  The result
    has the volume's dtype (uint8: sat8 of the f32 filter on the bytes).  W must be a multiple of 4; calls that share a plan are
    ordered by the caller (one stream).
    differentiable=False (the default): the result carries no grad_fn whatever the inputs require.  differentiable=True, with
    torch's grad mode on and a volume or a guide that requires a gradient: the call goes through `SmoothPlan.apply` on a cached
    `SmoothPlan.volume(..., differentiable=True)` -- same values, bit for bit; f32 volumes, and an f32 guide where the guide requires
    a gradient (TypeError otherwise); gradients with respect to the volume and the guide, all of it in the library, through the
    distances where the guide, or a self-guiding volume, requires one.  sigma_s and sigma_r may then be float tensors of one element,
    which receive gradients (one cached plan for every value; reading a sigma tensor costs one host read per call).  No gradient of
    spacing_z here; no double backward."""
    return _smooth_by_plan(volume, guide, sigma_s, sigma_r, iterations, differentiable, nd=3, spacing_z=spacing_z)


_SMOOTH_SCANS = [(0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1)]      # +x -x on weights 0, +y -y on weights 1


def edge_aware_smooth(image, guide=None, sigma_s: float = 60.0, sigma_r: float = 0.4, iterations: int = 3, form: str = "planes",
                      differentiable: bool = False):
    """Edge-aware smoothing of a device image (C, H, W) or (H, W), f32, by the domain-transform recursive filter: per iteration
    +x, -x on that iteration's x weights, then +y, -y on its y weights (two fused stages, six launches).  guide=None: the image
    guides itself.  One plan per (shape, device), cached; calls on one shape are ordered by the caller (one stream).
    form="plan" also takes a batch: image (N, C, H, W) with guide (N, G, H, W) or None, through a cached SmoothPlan(batch=N) -- every
    launch takes all N images, each filtered with its own edges, bit for bit as the 3-D call filters it; the other forms refuse 4-D.
    form="planes": the weight planes of `domain_transform_weights`, 2 per iteration, read by `execute`.  form="power": the two
    planes of `domain_transform_distances`, computed once, and `execute_power` with bases [a_k, a_k] per iteration -- no weight
    plane is stored; the guide may be uint8 (taken as it is: guide / 255).  form="plan": what "power" computes, by a cached
    SmoothPlan (keyed by shape, dtypes, iterations, sigmas and device) that owns the distance planes; the result has the image's
    dtype -- a uint8 image gives uint8 (sat8 of the f32 filter on the bytes, the byte image guiding itself as image / 255).
    Gradients: with form="planes", torch's grad mode on and an image or a guide that requires a gradient, the scans go through
    `var_scan` (same values, bit for bit) and the result is differentiable with respect to both -- the guide through the torch
    expression `domain_transform_weights` is.  form="plan" with differentiable=True goes through `SmoothPlan.apply` (same values,
    bit for bit): f32 images, gradients with respect to the image and an f32 guide, all of it in the library (through the
    distances where the guide, or a self-guiding image, requires a gradient).  Without the flag form="plan" carries no grad_fn
    whatever the inputs require, and form="power" never does: differentiable=True with form="power" raises ValueError (use
    "plan"); with form="planes" the flag changes nothing.  With form="plan" and differentiable=True, sigma_s and sigma_r may be float
    tensors of one element: they receive gradients (`SmoothPlan.backward_sigmas`), the plan cache key leaves the sigmas out, and
    reading a sigma tensor costs one host read per call.  Float sigmas take exactly the path they took."""
    import torch
    if form not in ("planes", "power", "plan"):
        raise ValueError(f"form must be 'planes', 'power' or 'plan', got {form!r}")
    if differentiable and form == "power":
        raise ValueError('form="power" is not differentiable: use form="plan" with differentiable=True (or form="planes")')
    if form == "plan":
        return _smooth_by_plan(image, guide, sigma_s, sigma_r, iterations, differentiable)
    img = image if image.dim() == 3 else image.unsqueeze(0)
    if img.dim() != 3:
        raise ValueError(f"image must be (C, H, W) or (H, W), got {tuple(image.shape)}")
    img = img.to(torch.float32).contiguous()
    if form == "planes" and torch.is_grad_enabled() and (image.requires_grad or (guide is not None and guide.requires_grad)):
        weights = domain_transform_weights(image if guide is None else guide, sigma_s, sigma_r, iterations)
        if tuple(weights[0][0].shape) != tuple(img.shape[1:]):
            raise ValueError("guide and image must have the same height and width")
        planes = [img[c] for c in range(img.shape[0])]
        with torch.cuda.device(img.device):
            for wx, wy in weights:
                planes = var_scan(planes, [wx.to(img.device), wy.to(img.device)], _SMOOTH_SCANS)
        out = torch.stack(list(planes))
        return out if image.dim() == 3 else out[0]
    if form == "power":
        g = img if guide is None else guide
        if g.dtype != torch.uint8:
            g = g.to(torch.float32)
        distances = [d.to(img.device) for d in domain_transform_distances(g.to(img.device), sigma_s, sigma_r)]
        weights = [(distances, [a_k, a_k]) for a_k in domain_transform_bases(sigma_s, iterations)]
        shape_hw = tuple(distances[0].shape)
    else:
        weights = domain_transform_weights(image if guide is None else guide, sigma_s, sigma_r, iterations)
        shape_hw = tuple(weights[0][0].shape)
    C, H, W = (int(s) for s in img.shape)
    if shape_hw != (H, W):
        raise ValueError("guide and image must have the same height and width")
    plan = _cached_plan(_smooth_plans, VarPlan, (H, W), _SMOOTH_SCANS, C, 2, _device_index(img))
    out = torch.empty_like(img)
    outs = [out[c] for c in range(C)]
    src = [img[c] for c in range(C)]
    for wx, wy in weights:
        if form == "power":
            plan.execute_power(src, wx, wy, outs)      # (the distance planes, this iteration's bases)
        else:
            plan.execute(src, [wx.to(img.device), wy.to(img.device)], outs)
        src = outs
    return out if image.dim() == 3 else out[0]
