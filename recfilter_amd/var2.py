"""Time-varying second-order all-pole scans on signals: thin Python handle over rf_var2_plan_* (include/recfilter_amd.h).

    causal      y[n] = x[n] - a1[n] y[n-1] - a2[n] y[n-2]          anticausal: the same on the three signals reversed

with coefficient signals as long as the input -- a resonator whose centre frequency and bandwidth move, an LPC synthesis filter,
the feedback half of a swept biquad.  The scans run in the HIP kernels of kernels_var2_signal.hip; torch tensors are device
memory.  `Var2Plan.backward` (rf_var2_plan_backward) is the adjoint in the same kernels' adjoint instances -- the gradient of the
input and, where asked for, of both coefficient signals -- and `Var2Plan.apply` / `allpole_scan` put it behind torch.autograd.
f32 only; no double backward.

The whole direct-form-I section runs on the same plans (rf_var2_plan_execute_biquad / _backward_biquad):

    v[n] = b0[n] x[n] + b1[n] x[n-1] + b2[n] x[n-2]          y[n] = v[n] - a1[n] y[n-1] - a2[n] y[n-2]

`Var2Plan.execute_biquad`, `backward_biquad` (the input's gradient and, where asked for, all five coefficient gradients),
`apply_biquad` and `biquad_scan` behind torch.autograd.

A cascade of K such sections, each with five coefficient signals of its own, runs in 2 K + 1 launches on one plan
(rf_var2_plan_execute_cascade / _backward_cascade): `Var2Plan.execute_cascade`, `backward_cascade`, `apply_cascade` and
`biquad_cascade`.  Autograd saves x, the coefficients and the result -- no intermediate signal: the backward reruns the sections
into signals the plan owns.  With keep=True the forward keeps every section's result in tensors autograd saves
(rf_var2_plan_execute_cascade_keep) and the backward reruns nothing (rf_var2_plan_backward_cascade_kept: one adjoint link launch
per boundary between two sections): `Var2Plan.execute_cascade_keep`, `backward_cascade_kept`.

The section also takes its coefficients at a control rate (rf_var2_plan_execute_biquad_frames / _backward_biquad_frames): one frame
every `hop` samples, a power of two from 64 to 65536, interpolated linearly in the kernels' registers -- `frames_count`,
`expand_frames`, `Var2Plan.execute_biquad_frames`, `backward_biquad_frames` (the input's gradient and, where asked for, the five
frame gradients, contracted in f64), `apply_biquad_frames` and `biquad_scan_frames` behind torch.autograd.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Sequence

from . import capi
from .capi import _PlanHandle, _timed


class Var2Plan(_PlanHandle):
    """One scan over `lines` f32 signals of `length` samples (a multiple of 4, up to 2**30), every line with coefficient signals of
    its own.  A signal argument is a device tensor of shape (length,) (lines == 1) or (lines, length) whose rows lie `stride`
    samples apart (default: length, a contiguous tensor; a wider stride is a [:, :length] view of a wider buffer).  Coefficients
    that would multiply a sample outside the line -- a1[0], a2[0], a2[1] of a causal scan, their mirror images of an anticausal
    one -- are never used.  One plan owns one workspace: order its calls."""
    _destroy = "rf_var2_plan_destroy"

    def __init__(self, length: int, lines: int = 1, causal: bool = True, device: int = -1, stride: int = None):
        d = capi.Var2SignalDesc()
        d.abi = capi.RF_ABI
        d.length, d.n_lines = int(length), int(lines)
        d.stride = int(length if stride is None else stride)
        d.causal = int(bool(causal))
        d.device, d.flags = int(device), 0
        self._desc = d
        self.length, self.lines, self.stride, self.causal = int(d.length), int(d.n_lines), int(d.stride), bool(causal)
        self._h = ctypes.c_void_p()
        capi.check(capi.lib().rf_var2_plan_create_signal(ctypes.byref(d), ctypes.byref(self._h)))

    # -- queries ----------------------------------------------------------------------------
    @property
    def workspace_bytes(self) -> int:
        """4 * lines * (6 * (tiles + groups) + 2 * groups), tiles = ceil(length / 64), groups = ceil(tiles / 64)"""
        return int(capi.lib().rf_var2_plan_workspace_bytes(self._h))

    @property
    def num_kernels(self) -> int:
        return int(capi.lib().rf_var2_plan_num_kernels(self._h))

    def backward_num_kernels(self, with_coefficients: bool = False) -> int:
        """3 launches, 4 with coefficient gradients"""
        return int(capi.lib().rf_var2_plan_backward_num_kernels(self._h, int(bool(with_coefficients))))

    # -- arguments ----------------------------------------------------------------------------
    @property
    def _host_only(self) -> bool:
        return self._desc.device == capi.RF_DEVICE_HOST_ONLY

    def _pointer(self, t, what: str) -> ctypes.c_void_p:
        """the address of a signal argument after its checks (None: a null pointer)"""
        import torch
        if t is None:
            return ctypes.c_void_p()
        shapes = [(self.lines, self.length)] + ([(self.length,)] if self.lines == 1 else [])
        if tuple(t.shape) not in shapes:
            raise ValueError(f"{what}: shape {tuple(t.shape)}, the plan takes {' or '.join(str(s) for s in shapes)}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: float32 signals only, got {t.dtype}")
        if not t.is_cuda or t.stride(-1) != 1 or (t.dim() == 2 and self.lines > 1 and t.stride(0) != self.stride):
            raise ValueError(f"{what}: a device tensor with dense rows {self.stride} samples apart")
        return ctypes.c_void_p(t.data_ptr())

    def _placeholders(self, count: int):
        """what a call on a host-only plan passes: there are no device tensors to take pointers from.  Addresses that pass the
        library's argument checks (16-byte aligned, apart) and are never dereferenced: the library refuses to run, RF_ERR_HIP"""
        span = ((self.lines - 1) * self.stride + self.length) * 4 + 4096
        return tuple(ctypes.c_void_p(4096 + i * span) for i in range(count))

    def _like(self, t):
        """a new tensor with the layout of `t` as this plan takes it"""
        import torch
        if self.lines > 1 and self.stride != self.length:
            return torch.empty((self.lines, self.stride), dtype=torch.float32, device=t.device)[:, :self.length]
        return torch.empty(tuple(t.shape), dtype=torch.float32, device=t.device)

    # -- execution --------------------------------------------------------------------------
    def _arguments(self, x, a1, a2, out, stream):
        if self._host_only:
            return self._placeholders(4) + (None, ctypes.c_void_p())
        if out is None:
            out = self._like(x)
        return (self._pointer(x, "x"), self._pointer(a1, "a1"), self._pointer(a2, "a2"), self._pointer(out, "out"), out, self._stream(stream))

    def execute(self, x, a1, a2, out=None, stream=None):
        """rf_var2_plan_execute: asynchronous on `stream` (default: torch's current stream).  out=None allocates the output; out may
        be x itself (in place)."""
        px, p1, p2, po, out, s = self._arguments(x, a1, a2, out, stream)
        capi.check(capi.lib().rf_var2_plan_execute(self._h, px, p1, p2, po, s))
        return out

    def execute_timed(self, x, a1, a2, out=None, stream=None):
        """rf_var2_plan_execute_timed: (output, [(kernel name, ms), ...]) measured with HIP events; synchronises the stream."""
        px, p1, p2, po, out, s = self._arguments(x, a1, a2, out, stream)
        return out, _timed(lambda *report: capi.lib().rf_var2_plan_execute_timed(self._h, px, p1, p2, po, s, *report), self.num_kernels)

    # -- the adjoint ------------------------------------------------------------------------
    def _backward_arguments(self, a1, a2, out, grad_out, grad_in, grad_a1, grad_a2, stream):
        if self._host_only:
            return self._placeholders(5) + (ctypes.c_void_p(), ctypes.c_void_p(), None, ctypes.c_void_p())
        if grad_in is None:
            grad_in = self._like(grad_out)
        return (self._pointer(a1, "a1"), self._pointer(a2, "a2"), self._pointer(out, "out"), self._pointer(grad_out, "grad_out"),
                self._pointer(grad_in, "grad_in"), self._pointer(grad_a1, "grad_a1"), self._pointer(grad_a2, "grad_a2"), grad_in,
                self._stream(stream))

    def backward(self, a1, a2, out, grad_out, grad_in=None, grad_a1=None, grad_a2=None, stream=None):
        """rf_var2_plan_backward, the adjoint of execute: grad_in = dL/dx from grad_out = dL/d(out); `out` is execute's result.
        grad_in=None allocates it; it may be grad_out itself (in place).  grad_a1 and grad_a2: both None (no coefficient gradients;
        `out` may then be None too) or both tensors to be WRITTEN.  Returns (grad_in, grad_a1, grad_a2).  Asynchronous; uses the
        plan's workspace like an execute."""
        p1, p2, po, pgo, pgi, pg1, pg2, grad_in, s = self._backward_arguments(a1, a2, out, grad_out, grad_in, grad_a1, grad_a2, stream)
        capi.check(capi.lib().rf_var2_plan_backward(self._h, p1, p2, po, pgo, pgi, pg1, pg2, s))
        return grad_in, grad_a1, grad_a2

    def backward_timed(self, a1, a2, out, grad_out, grad_in=None, grad_a1=None, grad_a2=None, stream=None):
        """rf_var2_plan_backward_timed: (grad_in, grad_a1, grad_a2, [(kernel name, ms), ...]); synchronises the stream."""
        p1, p2, po, pgo, pgi, pg1, pg2, grad_in, s = self._backward_arguments(a1, a2, out, grad_out, grad_in, grad_a1, grad_a2, stream)
        n = self.backward_num_kernels(grad_a1 is not None or grad_a2 is not None)
        times = _timed(lambda *report: capi.lib().rf_var2_plan_backward_timed(self._h, p1, p2, po, pgo, pgi, pg1, pg2, s, *report), n)
        return grad_in, grad_a1, grad_a2, times

    def apply(self, x, a1, a2):
        """execute, out of place, as a differentiable torch operation: the values are bit for bit execute's.  Backward is `backward`
        -- the input's gradient always, both coefficient gradients where either coefficient signal requires one.  The coefficients
        and the result are saved; no double backward."""
        return _function().apply(self, x, a1, a2)

    # -- the whole section, direct form I ---------------------------------------------------------
    #     v[n] = b0[n] x[n] + b1[n] x[n-1] + b2[n] x[n-2]        y[n] = v[n] - a1[n] y[n-1] - a2[n] y[n-2]
    @property
    def biquad_num_kernels(self) -> int:
        return int(capi.lib().rf_var2_plan_biquad_num_kernels(self._h))

    @property
    def backward_biquad_num_kernels(self) -> int:
        """4 launches, with or without coefficient gradients"""
        return int(capi.lib().rf_var2_plan_backward_biquad_num_kernels(self._h))

    @property
    def backward_biquad_bytes(self) -> int:
        """the adjoint state's signal the plan allocates in its first backward_biquad: 4 * ((lines - 1) * stride + length)"""
        return int(capi.lib().rf_var2_plan_backward_biquad_bytes(self._h))

    def _biquad_arguments(self, x, b0, b1, b2, a1, a2, out, stream):
        if self._host_only:
            return self._placeholders(7) + (None, ctypes.c_void_p())
        if out is None:
            out = self._like(x)
        names = ("x", "b0", "b1", "b2", "a1", "a2", "out")
        return tuple(self._pointer(t, w) for t, w in zip((x, b0, b1, b2, a1, a2, out), names)) + (out, self._stream(stream))

    def execute_biquad(self, x, b0, b1, b2, a1, a2, out=None, stream=None):
        """rf_var2_plan_execute_biquad: asynchronous on `stream` (default: torch's current stream).  out=None allocates the output;
        out may NOT be x (the first launch stores the feed-forward part while neighbouring groups still read x)."""
        *p, out, s = self._biquad_arguments(x, b0, b1, b2, a1, a2, out, stream)
        capi.check(capi.lib().rf_var2_plan_execute_biquad(self._h, *p, s))
        return out

    def execute_biquad_timed(self, x, b0, b1, b2, a1, a2, out=None, stream=None):
        """rf_var2_plan_execute_biquad_timed: (output, [(kernel name, ms), ...]); synchronises the stream."""
        *p, out, s = self._biquad_arguments(x, b0, b1, b2, a1, a2, out, stream)
        return out, _timed(lambda *report: capi.lib().rf_var2_plan_execute_biquad_timed(self._h, *p, s, *report), self.biquad_num_kernels)

    def _backward_biquad_arguments(self, x, b0, b1, b2, a1, a2, out, grad_out, grad_in, grads, stream):
        if grads is not None and len(grads) != 5:
            raise ValueError("grads: the five coefficient gradients (grad_b0, grad_b1, grad_b2, grad_a1, grad_a2) or None")
        if self._host_only:
            return self._placeholders(9) + (ctypes.c_void_p(),) * 5 + (None, grads, ctypes.c_void_p())
        if grad_in is None:
            grad_in = self._like(grad_out)
        names = ("x", "b0", "b1", "b2", "a1", "a2", "out", "grad_out", "grad_in", "grad_b0", "grad_b1", "grad_b2", "grad_a1", "grad_a2")
        tensors = (x, b0, b1, b2, a1, a2, out, grad_out, grad_in) + (tuple(grads) if grads is not None else (None,) * 5)
        return tuple(self._pointer(t, w) for t, w in zip(tensors, names)) + (grad_in, grads, self._stream(stream))

    def backward_biquad(self, x, b0, b1, b2, a1, a2, out, grad_out, grad_in=None, grads=None, stream=None):
        """rf_var2_plan_backward_biquad, the adjoint of execute_biquad: grad_in = dL/dx from grad_out = dL/d(out); `out` is
        execute_biquad's result.  grad_in=None allocates it; it may be grad_out itself.  grads: None (no coefficient gradients; `out`
        may then be None too) or the five tensors (grad_b0, grad_b1, grad_b2, grad_a1, grad_a2) to be WRITTEN.  Returns
        (grad_in, grads).  Asynchronous; uses the plan's workspace and its adjoint-state signal (allocated by the first call)."""
        *p, grad_in, grads, s = self._backward_biquad_arguments(x, b0, b1, b2, a1, a2, out, grad_out, grad_in, grads, stream)
        capi.check(capi.lib().rf_var2_plan_backward_biquad(self._h, *p, s))
        return grad_in, grads

    def backward_biquad_timed(self, x, b0, b1, b2, a1, a2, out, grad_out, grad_in=None, grads=None, stream=None):
        """rf_var2_plan_backward_biquad_timed: (grad_in, grads, [(kernel name, ms), ...]); synchronises the stream."""
        *p, grad_in, grads, s = self._backward_biquad_arguments(x, b0, b1, b2, a1, a2, out, grad_out, grad_in, grads, stream)
        times = _timed(lambda *report: capi.lib().rf_var2_plan_backward_biquad_timed(self._h, *p, s, *report), self.backward_biquad_num_kernels)
        return grad_in, grads, times

    def apply_biquad(self, x, b0, b1, b2, a1, a2):
        """execute_biquad as a differentiable torch operation: the values are bit for bit execute_biquad's.  Backward is
        backward_biquad -- the input's gradient always, the five coefficient gradients where any coefficient signal requires one.
        x, the five coefficients and the result are saved (no intermediate is); no double backward."""
        return _biquad_function().apply(self, x, b0, b1, b2, a1, a2)

    # -- the section on control-rate frames ---------------------------------------------------------
    #     frames: (b0, b1, b2, a1, a2), each (F,) (lines == 1) or (lines, F), F = frames_count(length, hop), frame j at sample
    #     j * hop; between two frames the coefficient is fma(k / hop, c[j+1] - c[j], c[j]), formed in the kernels' registers
    @property
    def biquad_frames_num_kernels(self) -> int:
        return int(capi.lib().rf_var2_plan_biquad_frames_num_kernels(self._h))

    def backward_biquad_frames_num_kernels(self, with_frames: bool = False) -> int:
        """4 launches, 5 with frame gradients (the fold)"""
        return int(capi.lib().rf_var2_plan_backward_biquad_frames_num_kernels(self._h, int(bool(with_frames))))

    def backward_biquad_frames_bytes(self, hop: int) -> int:
        """what the plan owns behind a backward_biquad_frames: lam and the slab of f64 partial sums, 80 bytes per piece of
        min(hop, 1024) samples"""
        return int(capi.lib().rf_var2_plan_backward_biquad_frames_bytes(self._h, int(hop)))

    def _frames_array(self, frames, hop: int, what: str, like=None):
        """(a one-element rf_var2_section array, n_frames, frame_stride) of five frame tensors after their checks; `like`: the
        frame stride they must share with (the gradients with the frames: the library takes one stride)"""
        import torch
        if frames is None:
            return None, 0, 0
        if len(frames) != 5:
            raise ValueError(f"{what}: the five frame tensors (b0, b1, b2, a1, a2)")
        count = frames_count(self.length, hop)
        shapes = [(self.lines, count)] + ([(count,)] if self.lines == 1 else [])
        array = (capi.Var2Section * 1)()
        stride = like
        for name, t in zip(("b0", "b1", "b2", "a1", "a2"), frames):
            if tuple(t.shape) not in shapes:
                raise ValueError(f"{what}.{name}: shape {tuple(t.shape)}, hop {hop} on this plan takes {' or '.join(str(s) for s in shapes)}")
            if t.dtype != torch.float32:
                raise TypeError(f"{what}.{name}: float32 frames only, got {t.dtype}")
            own = t.stride(0) if t.dim() == 2 and self.lines > 1 else count
            stride = own if stride is None else stride
            if not t.is_cuda or t.stride(-1) != 1 or own != stride:
                raise ValueError(f"{what}.{name}: a device tensor with dense rows, all five the same distance apart")
            setattr(array[0], name, t.data_ptr())
        return array, count, stride

    def _host_frames(self, hop: int, first: int):
        count = int(capi.lib().rf_var2_frames_count(self.length, int(hop)))
        p = self._placeholders(first + 5)
        return p[:first], (capi.Var2Section * 1)(capi.Var2Section(*(q.value for q in p[first:]))), count, count

    def _biquad_frames_arguments(self, x, frames, hop, out, stream):
        if self._host_only:
            (px, po), array, count, stride = self._host_frames(hop, 2)
            return px, array, int(hop), count, stride, po, None, ctypes.c_void_p()
        if out is None:
            out = self._like(x)
        array, count, stride = self._frames_array(frames, hop, "frames")
        return self._pointer(x, "x"), array, int(hop), count, stride, self._pointer(out, "out"), out, self._stream(stream)

    def execute_biquad_frames(self, x, frames, hop: int, out=None, stream=None):
        """rf_var2_plan_execute_biquad_frames: execute_biquad with the five coefficients as frames every `hop` samples (a power of
        two, 64..65536), bit for bit what execute_biquad gives on expand_frames of each.  out=None allocates the output; out may
        NOT be x.  Asynchronous on `stream` (default: torch's current stream)."""
        *p, out, s = self._biquad_frames_arguments(x, frames, hop, out, stream)
        capi.check(capi.lib().rf_var2_plan_execute_biquad_frames(self._h, *p, s))
        return out

    def execute_biquad_frames_timed(self, x, frames, hop: int, out=None, stream=None):
        """rf_var2_plan_execute_biquad_frames_timed: (output, [(kernel name, ms), ...]); synchronises the stream."""
        *p, out, s = self._biquad_frames_arguments(x, frames, hop, out, stream)
        call = lambda *report: capi.lib().rf_var2_plan_execute_biquad_frames_timed(self._h, *p, s, *report)      # noqa: E731
        return out, _timed(call, self.biquad_frames_num_kernels)

    def _backward_biquad_frames_arguments(self, x, frames, hop, out, grad_out, grad_in, grads, stream):
        if self._host_only:
            (px, po, pgo, pgi), array, count, stride = self._host_frames(hop, 4)
            return px, array, int(hop), count, stride, po, pgo, pgi, None, None, grads, ctypes.c_void_p()
        if grad_in is None:
            grad_in = self._like(grad_out)
        array, count, stride = self._frames_array(frames, hop, "frames")
        garray, _, _ = self._frames_array(grads, hop, "grads", like=stride)
        return (self._pointer(x, "x"), array, int(hop), count, stride, self._pointer(out, "out"), self._pointer(grad_out, "grad_out"),
                self._pointer(grad_in, "grad_in"), garray, grad_in, grads, self._stream(stream))

    def backward_biquad_frames(self, x, frames, hop: int, out, grad_out, grad_in=None, grads=None, stream=None):
        """rf_var2_plan_backward_biquad_frames, the adjoint of execute_biquad_frames: grad_in = dL/dx from grad_out; `out` is the
        forward's result.  grads: None (no frame gradients; `out` may then be None too) or five tensors laid out like the frames
        (the same distance between rows) to be WRITTEN: dL/d(frame), the per-sample gradients contracted in f64 with the
        interpolation's transpose and rounded once.  Returns (grad_in, grads).  Asynchronous; the plan allocates the adjoint
        state and the slab of partial sums in its first call (backward_biquad_frames_bytes)."""
        *p, grad_in, grads, s = self._backward_biquad_frames_arguments(x, frames, hop, out, grad_out, grad_in, grads, stream)
        capi.check(capi.lib().rf_var2_plan_backward_biquad_frames(self._h, *p, s))
        return grad_in, grads

    def backward_biquad_frames_timed(self, x, frames, hop: int, out, grad_out, grad_in=None, grads=None, stream=None):
        """rf_var2_plan_backward_biquad_frames_timed: (grad_in, grads, [(kernel name, ms), ...]); synchronises the stream."""
        *p, grad_in, grads, s = self._backward_biquad_frames_arguments(x, frames, hop, out, grad_out, grad_in, grads, stream)
        call = lambda *report: capi.lib().rf_var2_plan_backward_biquad_frames_timed(self._h, *p, s, *report)      # noqa: E731
        return grad_in, grads, _timed(call, self.backward_biquad_frames_num_kernels(grads is not None))

    def apply_biquad_frames(self, x, frames, hop: int):
        """execute_biquad_frames as a differentiable torch operation: the values are bit for bit execute_biquad_frames'.  Backward
        is backward_biquad_frames -- the input's gradient always, the five frame gradients where any frame tensor requires one.
        x, the frames and the result are saved; no double backward."""
        return _biquad_frames_function().apply(self, int(hop), x, *frames)


    # -- a cascade of sections ------------------------------------------------------------------
    #     sections: K tuples (b0, b1, b2, a1, a2), 1 <= K <= 16; section k + 1 runs on the result of section k, all in the plan's direction
    def cascade_num_kernels(self, sections: int) -> int:
        """2 K + 1 launches"""
        return int(capi.lib().rf_var2_plan_cascade_num_kernels(self._h, int(sections)))

    def backward_cascade_num_kernels(self, sections: int) -> int:
        """4 launches at K = 1, 6 K - 1 above: the rerun of K - 1 sections, then four launches per section"""
        return int(capi.lib().rf_var2_plan_backward_cascade_num_kernels(self._h, int(sections)))

    def backward_cascade_bytes(self, sections: int) -> int:
        """what the plan owns behind a backward_cascade of K sections: 1 span at K = 1, K + 1 above, of 4 * ((lines - 1) * stride + length)"""
        return int(capi.lib().rf_var2_plan_backward_cascade_bytes(self._h, int(sections)))

    def _section_array(self, sections, what: str):
        """(the rf_var2_section array or None, K).  Host-only: addresses that pass the library's checks, never dereferenced"""
        if sections is None:
            return None, 0
        K = len(sections)
        array = (capi.Var2Section * max(K, 1))()
        for k, s in enumerate(sections):
            if len(s) != 5:
                raise ValueError(f"{what}[{k}]: the five signals (b0, b1, b2, a1, a2)")
            for name, t in zip(("b0", "b1", "b2", "a1", "a2"), s):
                setattr(array[k], name, self._pointer(t, f"{what}[{k}].{name}").value)
        return array, K

    def _cascade_arguments(self, x, sections, out, stream):
        if self._host_only:
            K = len(sections)
            p = self._placeholders(2 + 5 * K)
            array = (capi.Var2Section * max(K, 1))(*(capi.Var2Section(*(q.value for q in p[2 + 5 * k:7 + 5 * k])) for k in range(K)))
            return p[0], array, K, p[1], None, ctypes.c_void_p()
        if out is None:
            out = self._like(x)
        array, K = self._section_array(sections, "sections")
        return self._pointer(x, "x"), array, K, self._pointer(out, "out"), out, self._stream(stream)

    def execute_cascade(self, x, sections: Sequence, out=None, stream=None):
        """rf_var2_plan_execute_cascade: asynchronous on `stream` (default: torch's current stream).  out=None allocates the output;
        out may NOT be x.  One section is execute_biquad's launches and bits."""
        px, array, K, po, out, s = self._cascade_arguments(x, sections, out, stream)
        capi.check(capi.lib().rf_var2_plan_execute_cascade(self._h, px, array, K, po, s))
        return out

    def execute_cascade_timed(self, x, sections: Sequence, out=None, stream=None):
        """rf_var2_plan_execute_cascade_timed: (output, [(kernel name, ms), ...]); synchronises the stream."""
        px, array, K, po, out, s = self._cascade_arguments(x, sections, out, stream)
        call = lambda *report: capi.lib().rf_var2_plan_execute_cascade_timed(self._h, px, array, K, po, s, *report)      # noqa: E731
        return out, _timed(call, self.cascade_num_kernels(K))

    def _backward_cascade_arguments(self, x, sections, out, grad_out, grad_in, grads, stream):
        if grads is not None and len(grads) != len(sections):
            raise ValueError("grads: one tuple (grad_b0, grad_b1, grad_b2, grad_a1, grad_a2) per section, or None")
        if self._host_only:
            K = len(sections)
            p = self._placeholders(4 + 5 * K)
            array = (capi.Var2Section * max(K, 1))(*(capi.Var2Section(*(q.value for q in p[4 + 5 * k:9 + 5 * k])) for k in range(K)))
            return p[0], array, K, p[1], p[2], p[3], None, None, grads, ctypes.c_void_p()
        if grad_in is None:
            grad_in = self._like(grad_out)
        array, K = self._section_array(sections, "sections")
        garray, _ = self._section_array(grads, "grads")
        return (self._pointer(x, "x"), array, K, self._pointer(out, "out"), self._pointer(grad_out, "grad_out"),
                self._pointer(grad_in, "grad_in"), garray, grad_in, grads, self._stream(stream))

    def backward_cascade(self, x, sections: Sequence, out, grad_out, grad_in=None, grads=None, stream=None):
        """rf_var2_plan_backward_cascade, the adjoint of execute_cascade: grad_in = dL/dx from grad_out = dL/d(out); `out` is
        execute_cascade's result.  grad_in=None allocates it; it may be grad_out itself.  grads: None (no coefficient gradients;
        `out` may then be None too) or K tuples of five tensors to be WRITTEN.  Returns (grad_in, grads).  Asynchronous; nothing is
        kept from the forward: the call reruns all sections but the last into signals of the plan's (backward_cascade_bytes)."""
        px, array, K, po, pgo, pgi, garray, grad_in, grads, s = self._backward_cascade_arguments(x, sections, out, grad_out, grad_in, grads, stream)
        capi.check(capi.lib().rf_var2_plan_backward_cascade(self._h, px, array, K, po, pgo, pgi, garray, s))
        return grad_in, grads

    def backward_cascade_timed(self, x, sections: Sequence, out, grad_out, grad_in=None, grads=None, stream=None):
        """rf_var2_plan_backward_cascade_timed: (grad_in, grads, [(kernel name, ms), ...]); synchronises the stream."""
        px, array, K, po, pgo, pgi, garray, grad_in, grads, s = self._backward_cascade_arguments(x, sections, out, grad_out, grad_in, grads, stream)
        call = lambda *report: capi.lib().rf_var2_plan_backward_cascade_timed(self._h, px, array, K, po, pgo, pgi, garray, s, *report)      # noqa: E731
        return grad_in, grads, _timed(call, self.backward_cascade_num_kernels(K))

    # -- the cascade for training: the forward keeps every section's result, the backward reruns nothing ----------------------
    def backward_cascade_kept_num_kernels(self, sections: int, with_coefficients: bool = False) -> int:
        """2 K + 2 launches without coefficient gradients, 3 K + 1 with them (4 at K = 1 either way)"""
        return int(capi.lib().rf_var2_plan_backward_cascade_kept_num_kernels(self._h, int(sections), int(bool(with_coefficients))))

    def backward_cascade_kept_bytes(self, sections: int) -> int:
        """what the plan owns behind a backward_cascade_kept: 1 span at K = 1 (lam), 2 above (lam and the gradient between
        sections), whatever K"""
        return int(capi.lib().rf_var2_plan_backward_cascade_kept_bytes(self._h, int(sections)))

    def _kept_array(self, kept, count: int):
        """the array of the kept signals' addresses (None: a null pointer)"""
        if kept is None:
            return None
        if len(kept) != count:
            raise ValueError(f"kept: one signal per section but the last ({count}), got {len(kept)}")
        return (ctypes.c_void_p * max(count, 1))(*(self._pointer(t, f"kept[{k}]").value for k, t in enumerate(kept)))

    def _cascade_keep_arguments(self, x, sections, out, kept, stream):
        K = len(sections)
        if self._host_only:
            p = self._placeholders(2 + 5 * K + K - 1)
            array = (capi.Var2Section * max(K, 1))(*(capi.Var2Section(*(q.value for q in p[2 + 5 * k:7 + 5 * k])) for k in range(K)))
            return p[0], array, K, p[1], (ctypes.c_void_p * max(K - 1, 1))(*(q.value for q in p[2 + 5 * K:])), None, None, ctypes.c_void_p()
        if out is None:
            out = self._like(x)
        if kept is None:
            kept = [self._like(x) for _ in range(K - 1)]
        array, K = self._section_array(sections, "sections")
        return self._pointer(x, "x"), array, K, self._pointer(out, "out"), self._kept_array(kept, max(K - 1, 0)), out, list(kept), self._stream(stream)

    def execute_cascade_keep(self, x, sections: Sequence, out=None, kept=None, stream=None):
        """rf_var2_plan_execute_cascade_keep: execute_cascade with every section's result kept.  Returns (out, kept): kept[k] is
        section k's result, K - 1 tensors laid out like x (kept=None allocates them); out is execute_cascade's bit for bit.  The
        kept signals are the caller's: the plan keeps no state between calls."""
        px, array, K, po, pk, out, kept, s = self._cascade_keep_arguments(x, sections, out, kept, stream)
        capi.check(capi.lib().rf_var2_plan_execute_cascade_keep(self._h, px, array, K, po, pk, s))
        return out, kept

    def execute_cascade_keep_timed(self, x, sections: Sequence, out=None, kept=None, stream=None):
        """rf_var2_plan_execute_cascade_keep_timed: (out, kept, [(kernel name, ms), ...]); synchronises the stream."""
        px, array, K, po, pk, out, kept, s = self._cascade_keep_arguments(x, sections, out, kept, stream)
        call = lambda *report: capi.lib().rf_var2_plan_execute_cascade_keep_timed(self._h, px, array, K, po, pk, s, *report)      # noqa: E731
        return out, kept, _timed(call, self.cascade_num_kernels(K))

    def _backward_cascade_kept_arguments(self, x, sections, kept, out, grad_out, grad_in, grads, stream):
        K = len(sections)
        if grads is not None and len(grads) != K:
            raise ValueError("grads: one tuple (grad_b0, grad_b1, grad_b2, grad_a1, grad_a2) per section, or None")
        if self._host_only:
            p = self._placeholders(4 + 5 * K + K - 1)
            array = (capi.Var2Section * max(K, 1))(*(capi.Var2Section(*(q.value for q in p[4 + 5 * k:9 + 5 * k])) for k in range(K)))
            pk = (ctypes.c_void_p * max(K - 1, 1))(*(q.value for q in p[4 + 5 * K:]))
            return p[0], array, K, pk, p[1], p[2], p[3], None, None, grads, ctypes.c_void_p()
        if grad_in is None:
            grad_in = self._like(grad_out)
        array, K = self._section_array(sections, "sections")
        garray, _ = self._section_array(grads, "grads")
        return (self._pointer(x, "x"), array, K, self._kept_array(kept, max(K - 1, 0)), self._pointer(out, "out"), self._pointer(grad_out, "grad_out"),
                self._pointer(grad_in, "grad_in"), garray, grad_in, grads, self._stream(stream))

    def backward_cascade_kept(self, x, sections: Sequence, kept, out, grad_out, grad_in=None, grads=None, stream=None):
        """rf_var2_plan_backward_cascade_kept, the adjoint of execute_cascade_keep on what it kept: nothing is rerun -- one adjoint
        link launch per boundary forms the gradient that enters the section before on the adjoint state in registers.  grads:
        None (no coefficient gradients: x, kept and out may then be None, nothing of the forward is read) or K tuples of five
        tensors to be WRITTEN.  grad_in=None allocates it; it may be grad_out itself.  Returns (grad_in, grads).  Asynchronous;
        uses the plan's workspace and one or two signals of its own (backward_cascade_kept_bytes)."""
        px, array, K, pk, po, pgo, pgi, garray, grad_in, grads, s = self._backward_cascade_kept_arguments(x, sections, kept, out, grad_out, grad_in, grads, stream)
        capi.check(capi.lib().rf_var2_plan_backward_cascade_kept(self._h, px, array, K, pk, po, pgo, pgi, garray, s))
        return grad_in, grads

    def backward_cascade_kept_timed(self, x, sections: Sequence, kept, out, grad_out, grad_in=None, grads=None, stream=None):
        """rf_var2_plan_backward_cascade_kept_timed: (grad_in, grads, [(kernel name, ms), ...]); synchronises the stream."""
        px, array, K, pk, po, pgo, pgi, garray, grad_in, grads, s = self._backward_cascade_kept_arguments(x, sections, kept, out, grad_out, grad_in, grads, stream)
        call = lambda *report: capi.lib().rf_var2_plan_backward_cascade_kept_timed(self._h, px, array, K, pk, po, pgo, pgi, garray, s, *report)      # noqa: E731
        return grad_in, grads, _timed(call, self.backward_cascade_kept_num_kernels(K, grads is not None))

    def apply_cascade(self, x, sections: Sequence, keep: bool = False):
        """execute_cascade as a differentiable torch operation: the values are bit for bit execute_cascade's.  Backward is
        backward_cascade -- the input's gradient always, all 5 K coefficient gradients where any coefficient signal requires one.
        x, the coefficients and the result are saved, no intermediate signal; no double backward.
        keep=True: the same values, and the backward is backward_cascade_kept.  Where a coefficient signal requires a gradient
        the forward is execute_cascade_keep and the K - 1 kept signals are saved beside x, the coefficients and the result; where
        only x does, the forward is execute_cascade and the coefficients alone are saved."""
        function = _cascade_kept_function() if keep else _cascade_function()
        return function.apply(self, x, *(t for s in sections for t in s))

    # -- a cascade of sections on control-rate frames ---------------------------------------------
    #     sections: K tuples of five FRAME tensors (b0, b1, b2, a1, a2), one hop for all; no coefficient signal exists
    def cascade_frames_num_kernels(self, sections: int) -> int:
        """2 K + 1 launches (3 at K = 1: execute_biquad_frames')"""
        return int(capi.lib().rf_var2_plan_cascade_frames_num_kernels(self._h, int(sections)))

    def backward_cascade_frames_num_kernels(self, sections: int, with_frames: bool = False) -> int:
        """2 K + 2 launches without frame gradients, 3 K + 2 with them; 4 and 5 at K = 1"""
        return int(capi.lib().rf_var2_plan_backward_cascade_frames_num_kernels(self._h, int(sections), int(bool(with_frames))))

    def backward_cascade_frames_bytes(self, sections: int, hop: int) -> int:
        """what the plan owns behind a backward_cascade_frames: lam, the gradient between sections (K >= 2) and K slabs of 80 bytes
        per piece of min(hop, 1024) samples; 0 for a refused K or hop"""
        return int(capi.lib().rf_var2_plan_backward_cascade_frames_bytes(self._h, int(sections), int(hop)))

    def _sections_frames(self, sections, hop: int, what: str, like=None):
        """(the rf_var2_section array of K sections' frames or None, K, n_frames, frame_stride): every tensor checked as
        _frames_array checks it, all of them one distance between rows"""
        if sections is None:
            return None, 0, 0, like
        K = len(sections)
        array = (capi.Var2Section * max(K, 1))()
        count, stride = frames_count(self.length, hop), like
        for k, s in enumerate(sections):
            one, count, stride = self._frames_array(s, hop, f"{what}[{k}]", like=stride)
            array[k] = one[0]
        return array, K, count, count if stride is None else stride      # (no section: the library refuses the count)

    def _host_sections_frames(self, K: int, hop: int, first: int, with_grads: bool = False):
        """a host-only plan's arguments: `first` signals, K sections' frames, K - 1 kept signals and, where asked for, K
        sections' frame gradients -- addresses that pass the library's checks and are never dereferenced"""
        count = int(capi.lib().rf_var2_frames_count(self.length, int(hop)))
        p = self._placeholders(first + 10 * K + max(K - 1, 0))
        sections = lambda at: (capi.Var2Section * max(K, 1))(      # noqa: E731
            *(capi.Var2Section(*(q.value for q in p[at + 5 * k:at + 5 * k + 5])) for k in range(K)))
        kept = (ctypes.c_void_p * max(K - 1, 1))(*(q.value for q in p[first + 5 * K:first + 5 * K + max(K - 1, 0)]))
        return p[:first], sections(first), kept, sections(first + 6 * K - 1) if with_grads else None, count, count

    def _cascade_frames_arguments(self, x, sections, hop, out, keep, kept, stream):
        K = len(sections)
        if self._host_only:
            (px, po), array, pk, _, count, stride = self._host_sections_frames(K, hop, 2)
            return px, array, K, int(hop), count, stride, po, pk if keep else None, None, None, ctypes.c_void_p()
        if out is None:
            out = self._like(x)
        if keep and kept is None:
            kept = [self._like(x) for _ in range(K - 1)]
        array, K, count, stride = self._sections_frames(sections, hop, "sections")
        pk = self._kept_array(kept, max(K - 1, 0)) if keep else None
        return (self._pointer(x, "x"), array, K, int(hop), count, stride, self._pointer(out, "out"), pk, out, list(kept) if keep else None,
                self._stream(stream))

    def execute_cascade_frames(self, x, sections: Sequence, hop: int, out=None, keep: bool = False, kept=None, stream=None):
        """rf_var2_plan_execute_cascade_frames: execute_cascade with every section's five coefficients as frames every `hop`
        samples, bit for bit what execute_cascade gives on expand_frames of each.  keep=True: returns (out, kept), kept[k]
        section k's result in K - 1 tensors laid out like x (kept=None allocates them); out has the same bits either way.
        out=None allocates the output; out may NOT be x.  One section is execute_biquad_frames' launches and bits."""
        *p, out, kept, s = self._cascade_frames_arguments(x, sections, hop, out, keep or kept is not None, kept, stream)
        capi.check(capi.lib().rf_var2_plan_execute_cascade_frames(self._h, *p, s))
        return (out, kept) if keep or kept is not None else out

    def execute_cascade_frames_timed(self, x, sections: Sequence, hop: int, out=None, keep: bool = False, kept=None, stream=None):
        """rf_var2_plan_execute_cascade_frames_timed: (out, [(kernel name, ms), ...]) or (out, kept, [...]); synchronises the stream."""
        *p, out, kept, s = self._cascade_frames_arguments(x, sections, hop, out, keep or kept is not None, kept, stream)
        call = lambda *report: capi.lib().rf_var2_plan_execute_cascade_frames_timed(self._h, *p, s, *report)      # noqa: E731
        times = _timed(call, self.cascade_frames_num_kernels(len(sections)))
        return (out, kept, times) if keep or kept is not None else (out, times)

    def _backward_cascade_frames_arguments(self, x, sections, hop, kept, out, grad_out, grad_in, grads, stream):
        K = len(sections)
        if grads is not None and len(grads) != K:
            raise ValueError("grads: one tuple of five frame gradients per section, or None")
        if self._host_only:
            (px, po, pgo, pgi), array, pk, garray, count, stride = self._host_sections_frames(K, hop, 4, grads is not None)
            return px, array, K, int(hop), count, stride, pk, po, pgo, pgi, garray, None, grads, ctypes.c_void_p()
        if grad_in is None:
            grad_in = self._like(grad_out)
        array, K, count, stride = self._sections_frames(sections, hop, "sections")
        garray, _, _, _ = self._sections_frames(grads, hop, "grads", like=stride)
        return (self._pointer(x, "x"), array, K, int(hop), count, stride, self._kept_array(kept, max(K - 1, 0)), self._pointer(out, "out"),
                self._pointer(grad_out, "grad_out"), self._pointer(grad_in, "grad_in"), garray, grad_in, grads, self._stream(stream))

    def backward_cascade_frames(self, x, sections: Sequence, hop: int, kept, out, grad_out, grad_in=None, grads=None, stream=None):
        """rf_var2_plan_backward_cascade_frames, the adjoint of execute_cascade_frames on what it kept: nothing is rerun.  grads:
        None (no frame gradients: x, kept and out may then be None) or K tuples of five tensors laid out like the frames to be
        WRITTEN: dL/d(frame), contracted in f64 and rounded once.  grad_in=None allocates it; it may be grad_out itself.  Returns
        (grad_in, grads).  Asynchronous; the plan owns lam, the gradient between sections and the slab (backward_cascade_frames_bytes)."""
        *p, grad_in, grads, s = self._backward_cascade_frames_arguments(x, sections, hop, kept, out, grad_out, grad_in, grads, stream)
        capi.check(capi.lib().rf_var2_plan_backward_cascade_frames(self._h, *p, s))
        return grad_in, grads

    def backward_cascade_frames_timed(self, x, sections: Sequence, hop: int, kept, out, grad_out, grad_in=None, grads=None, stream=None):
        """rf_var2_plan_backward_cascade_frames_timed: (grad_in, grads, [(kernel name, ms), ...]); synchronises the stream."""
        *p, grad_in, grads, s = self._backward_cascade_frames_arguments(x, sections, hop, kept, out, grad_out, grad_in, grads, stream)
        call = lambda *report: capi.lib().rf_var2_plan_backward_cascade_frames_timed(self._h, *p, s, *report)      # noqa: E731
        return grad_in, grads, _timed(call, self.backward_cascade_frames_num_kernels(len(sections), grads is not None))

    def apply_cascade_frames(self, x, sections: Sequence, hop: int):
        """execute_cascade_frames as a differentiable torch operation: the values are bit for bit execute_cascade_frames'.  Backward
        is backward_cascade_frames.  Where any frame tensor requires a gradient the forward keeps, and x, the frames, the result
        and the K - 1 kept signals are saved; where only x does, the plain forward runs and the frames alone are saved."""
        return _cascade_frames_function().apply(self, int(hop), x, *(t for s in sections for t in s))

    # -- the cascade on frames with a state that enters and leaves the call --------------------------
    #     state: (K + 1, 2) (lines == 1) or (lines, K + 1, 2): pair 0 the input's history, pair k + 1 section k's result's, each
    #     (one place before the line, two places before it) in the direction of the recurrence
    def cascade_frames_stream_num_kernels(self, sections: int) -> int:
        """2 K + 1 launches, K = 1 included"""
        return int(capi.lib().rf_var2_plan_cascade_frames_stream_num_kernels(self._h, int(sections)))

    def cascade_frames_stream_state_bytes(self, sections: int, state_stride: int = None) -> int:
        """the bytes of one state buffer, 4 ((lines - 1) state_stride + 2 (K + 1)); state_stride defaults to 2 (K + 1); 0 for a
        refused K or stride"""
        stride = 2 * (int(sections) + 1) if state_stride is None else int(state_stride)
        return int(capi.lib().rf_var2_plan_cascade_frames_stream_state_bytes(self._h, int(sections), stride))

    def _state_pointer(self, t, K: int, what: str, stride=None):
        """(the address of a state tensor after its checks, the distance between lines).  The state buffers of one call share one
        distance: `stride` is what the buffers before this one fixed (None: none was given yet), a tensor with another raises,
        and a null one (None) passes it on -- so the calls chain this function over their buffers and the rule holds whichever
        of them are given."""
        import torch
        pairs = 2 * (K + 1)
        if t is None:
            return ctypes.c_void_p(), stride
        shapes = [(self.lines, K + 1, 2)] + ([(K + 1, 2)] if self.lines == 1 else [])
        if tuple(t.shape) not in shapes:
            raise ValueError(f"{what}: shape {tuple(t.shape)}, {K} sections on this plan take {' or '.join(str(s) for s in shapes)}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: float32 states only, got {t.dtype}")
        own = int(t.stride(0)) if t.dim() == 3 and self.lines > 1 else pairs
        if not t.is_cuda or t.stride(-1) != 1 or t.stride(-2) != 2 or (stride is not None and own != stride):
            raise ValueError(f"{what}: a device tensor with dense (K + 1, 2) blocks, state and state_out the same distance apart")
        return ctypes.c_void_p(t.data_ptr()), own

    @staticmethod
    def _dense_state_stride(stride, K: int) -> int:
        """the distance the library is handed: what the buffers fixed, or dense where none was given"""
        return 2 * (K + 1) if stride is None else stride

    def _cascade_frames_stream_arguments(self, x, sections, hop, state, out, keep, kept, state_out, stream):
        K = len(sections)
        if self._host_only:
            (px, po, psi, pso), array, pk, _, count, stride = self._host_sections_frames(K, hop, 4)
            null = ctypes.c_void_p()
            return (px, array, K, int(hop), count, stride, po, pk if keep else None, psi if state is not None else null,
                    pso if state_out is not False else null, 2 * (K + 1), None, None, None, null)
        import torch
        *p, out, kept, s = self._cascade_frames_arguments(x, sections, hop, out, keep, kept, stream)
        psi, stride = self._state_pointer(state, K, "state")
        if state_out is None:
            shape = (K + 1, 2) if x.dim() == 1 else (self.lines, K + 1, 2)
            state_out = (torch.empty_strided(tuple(state.shape), state.stride(), dtype=torch.float32, device=x.device) if state is not None
                         else torch.empty(shape, dtype=torch.float32, device=x.device))
        elif state_out is False:
            state_out = None
        pso, stride = self._state_pointer(state_out, K, "state_out", stride)
        return (*p, psi, pso, self._dense_state_stride(stride, K), out, kept, state_out, s)

    def execute_cascade_frames_stream(self, x, sections: Sequence, hop: int, state=None, out=None, keep: bool = False, kept=None,
                                      state_out=None, stream=None):
        """rf_var2_plan_execute_cascade_frames_stream: execute_cascade_frames on one chunk of a longer signal.  `state` enters (None:
        silence) and the state that leaves is returned: (out, state_out), or (out, kept, state_out) where keeping.  `sections`
        holds the CHUNK's frames -- for a chunk that starts at sample s of the whole signal, a multiple of hop, the slice
        [..., s // hop : s // hop + frames_count(length, hop)] of the whole signal's.  An anticausal plan takes its chunks last to
        first.  state_out: a tensor to be written (apart from `state`), None allocates it, False: not wanted (None is returned;
        with state=None too the call is execute_cascade_frames itself).  The plan keeps no state."""
        *p, out, kept, state_out, s = self._cascade_frames_stream_arguments(x, sections, hop, state, out, keep or kept is not None, kept, state_out, stream)
        capi.check(capi.lib().rf_var2_plan_execute_cascade_frames_stream(self._h, *p, s))
        return (out, kept, state_out) if keep or kept is not None else (out, state_out)

    def execute_cascade_frames_stream_timed(self, x, sections: Sequence, hop: int, state=None, out=None, keep: bool = False, kept=None,
                                            state_out=None, stream=None):
        """rf_var2_plan_execute_cascade_frames_stream_timed: execute_cascade_frames_stream's results and [(kernel name, ms), ...]
        behind them; synchronises the stream."""
        *p, out, kept, state_out, s = self._cascade_frames_stream_arguments(x, sections, hop, state, out, keep or kept is not None, kept, state_out, stream)
        call = lambda *report: capi.lib().rf_var2_plan_execute_cascade_frames_stream_timed(self._h, *p, s, *report)      # noqa: E731
        streamed = state is not None or state_out is not None
        times = _timed(call, self.cascade_frames_stream_num_kernels(len(sections)) if streamed else self.cascade_frames_num_kernels(len(sections)))
        return (out, kept, state_out, times) if keep or kept is not None else (out, state_out, times)

    def backward_cascade_frames_stream_num_kernels(self, sections: int, with_frames: bool = False) -> int:
        """2 K + 2 launches without frame gradients, 3 K + 2 with them, K = 1 included"""
        return int(capi.lib().rf_var2_plan_backward_cascade_frames_stream_num_kernels(self._h, int(sections), int(bool(with_frames))))

    def _backward_cascade_frames_stream_arguments(self, x, sections, hop, kept, out, grad_out, grad_in, grads, state, grad_state_out, grad_state_in, stream):
        K = len(sections)
        *p, grad_in, grads, s = self._backward_cascade_frames_arguments(x, sections, hop, kept, out, grad_out, grad_in, grads, stream)
        if self._host_only:
            psi, pgo, pgi = self._placeholders(7 + 11 * K)[-3:]
            null = ctypes.c_void_p()
            return (*p, psi if state is not None else null, pgo if grad_state_out is not None else null, pgi if grad_state_in is not False else null,
                    2 * (K + 1), None, grads, None, null)
        import torch
        psi, stride = self._state_pointer(state, K, "state")
        pgo, stride = self._state_pointer(grad_state_out, K, "grad_state_out", stride)
        like = state if state is not None else grad_state_out      # what a grad_state_in allocated here is laid out like
        if grad_state_in is None:
            shape = (K + 1, 2) if grad_out.dim() == 1 else (self.lines, K + 1, 2)
            grad_state_in = (torch.empty_strided(tuple(like.shape), like.stride(), dtype=torch.float32, device=grad_out.device) if like is not None
                             else torch.empty(shape, dtype=torch.float32, device=grad_out.device))
        elif grad_state_in is False:
            grad_state_in = None
        pgi, stride = self._state_pointer(grad_state_in, K, "grad_state_in", stride)
        return (*p, psi, pgo, pgi, self._dense_state_stride(stride, K), grad_in, grads, grad_state_in, s)

    def backward_cascade_frames_stream(self, x, sections: Sequence, hop: int, kept, out, grad_out, grad_in=None, grads=None, state=None,
                                       grad_state_out=None, grad_state_in=None, stream=None):
        """rf_var2_plan_backward_cascade_frames_stream, the adjoint of execute_cascade_frames_stream on what it kept: backward_cascade_frames'
        arguments, then `state` (what entered the forward; read for the frame gradients alone), grad_state_out (the gradient of the
        state that left; None: zeros) and grad_state_in (a tensor to be WRITTEN, None allocates it, False: not wanted).  Returns
        (grad_in, grads, grad_state_in)."""
        *p, grad_in, grads, grad_state_in, s = self._backward_cascade_frames_stream_arguments(x, sections, hop, kept, out, grad_out, grad_in, grads, state,
                                                                                              grad_state_out, grad_state_in, stream)
        capi.check(capi.lib().rf_var2_plan_backward_cascade_frames_stream(self._h, *p, s))
        return grad_in, grads, grad_state_in

    def backward_cascade_frames_stream_timed(self, x, sections: Sequence, hop: int, kept, out, grad_out, grad_in=None, grads=None, state=None,
                                             grad_state_out=None, grad_state_in=None, stream=None):
        """rf_var2_plan_backward_cascade_frames_stream_timed: (grad_in, grads, grad_state_in, [(kernel name, ms), ...]); synchronises the stream."""
        streamed = state is not None or grad_state_out is not None or grad_state_in is not False
        *p, grad_in, grads, grad_state_in, s = self._backward_cascade_frames_stream_arguments(x, sections, hop, kept, out, grad_out, grad_in, grads, state,
                                                                                              grad_state_out, grad_state_in, stream)
        call = lambda *report: capi.lib().rf_var2_plan_backward_cascade_frames_stream_timed(self._h, *p, s, *report)      # noqa: E731
        count = (self.backward_cascade_frames_stream_num_kernels if streamed else self.backward_cascade_frames_num_kernels)(len(sections), grads is not None)
        return grad_in, grads, grad_state_in, _timed(call, count)

    def apply_cascade_frames_stream(self, x, sections: Sequence, hop: int, state=None):
        """execute_cascade_frames_stream as a differentiable torch operation: (out, state), the values bit for bit that call's.
        Differentiable in x, in all 5 K frame tensors and in `state`, and a gradient may flow into the returned state (the next
        chunk's): backward is backward_cascade_frames_stream.  Where a frame tensor requires a gradient the forward keeps, and x,
        the frames, the state, the result and the K - 1 kept signals are saved; otherwise the frames alone."""
        return _cascade_frames_stream_function().apply(self, int(hop), x, state, *(t for s in sections for t in s))



_var2_function = None
_var2_biquad_function = None
_var2_cascade_function = None
_var2_cascade_kept_function = None


def _cascade_kept_function():
    """the torch.autograd.Function behind Var2Plan.apply_cascade(keep=True): (plan, x, then the 5 K coefficient signals)"""
    global _var2_cascade_kept_function
    if _var2_cascade_kept_function is not None:
        return _var2_cascade_kept_function
    import torch

    class Var2CascadeKeptFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, x, *coefficients):
            ctx.plan = plan
            sections = [coefficients[i:i + 5] for i in range(0, len(coefficients), 5)]
            ctx.with_coefficients = any(ctx.needs_input_grad[2:])
            with torch.cuda.device(x.device):
                if ctx.with_coefficients:
                    out, kept = plan.execute_cascade_keep(x, sections)
                    ctx.save_for_backward(x, *coefficients, out, *kept)
                else:      # the backward reads nothing of the forward
                    out = plan.execute_cascade(x, sections)
                    ctx.save_for_backward(*coefficients)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            plan = ctx.plan
            need_x, *need = ctx.needs_input_grad[1:]
            count = len(need)
            if ctx.with_coefficients:
                x, *rest = ctx.saved_tensors
                coefficients, out, kept = rest[:count], rest[count], rest[count + 1:]
            else:
                x, coefficients, out, kept = None, ctx.saved_tensors, None, None
            sections = [coefficients[i:i + 5] for i in range(0, count, 5)]
            g = _plan_layout(plan, grad_out)
            grads = [tuple(plan._like(g) for _ in range(5)) for _ in sections] if ctx.with_coefficients else None
            with torch.cuda.device(g.device):
                gin, grads = plan.backward_cascade_kept(x, sections, kept, out, g, None, grads)
            given = [t for s in grads for t in s] if grads is not None else [None] * count
            return (None, gin if need_x else None) + tuple(t if wanted else None for t, wanted in zip(given, need))

    _var2_cascade_kept_function = Var2CascadeKeptFunction
    return _var2_cascade_kept_function


def _cascade_function():
    """the torch.autograd.Function behind Var2Plan.apply_cascade: (plan, x, then the 5 K coefficient signals section by section)"""
    global _var2_cascade_function
    if _var2_cascade_function is not None:
        return _var2_cascade_function
    import torch

    class Var2CascadeFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, x, *coefficients):
            ctx.plan = plan
            sections = [coefficients[i:i + 5] for i in range(0, len(coefficients), 5)]
            with torch.cuda.device(x.device):
                out = plan.execute_cascade(x, sections)
            ctx.save_for_backward(x, *coefficients, out)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            plan = ctx.plan
            x, *coefficients, out = ctx.saved_tensors
            sections = [coefficients[i:i + 5] for i in range(0, len(coefficients), 5)]
            need_x, *need = ctx.needs_input_grad[1:]
            g = _plan_layout(plan, grad_out)
            grads = [tuple(plan._like(g) for _ in range(5)) for _ in sections] if any(need) else None
            with torch.cuda.device(g.device):
                gin, grads = plan.backward_cascade(x, sections, out, g, None, grads)
            given = [t for s in grads for t in s] if grads is not None else [None] * len(coefficients)
            return (None, gin if need_x else None) + tuple(t if wanted else None for t, wanted in zip(given, need))

    _var2_cascade_function = Var2CascadeFunction
    return _var2_cascade_function


_var2_biquad_frames_function = None
_var2_cascade_frames_function = None
_var2_cascade_frames_stream_function = None


def _cascade_frames_stream_function():
    """the torch.autograd.Function behind Var2Plan.apply_cascade_frames_stream: (plan, hop, x, state or None, then the 5 K frame
    tensors) -> (out, the state that leaves)"""
    global _var2_cascade_frames_stream_function
    if _var2_cascade_frames_stream_function is not None:
        return _var2_cascade_frames_stream_function
    import torch

    class Var2CascadeFramesStreamFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, hop, x, state, *frames):
            ctx.plan, ctx.hop, ctx.has_state = plan, hop, state is not None
            sections = [frames[i:i + 5] for i in range(0, len(frames), 5)]
            ctx.with_frames = any(ctx.needs_input_grad[4:])
            with torch.cuda.device(x.device):
                if ctx.with_frames:
                    out, kept, leaving = plan.execute_cascade_frames_stream(x, sections, hop, state, keep=True)
                    ctx.save_for_backward(x, *frames, out, *kept, *([state] if state is not None else []))
                else:      # the backward reads nothing of the forward
                    out, leaving = plan.execute_cascade_frames_stream(x, sections, hop, state)
                    ctx.save_for_backward(*frames)
            ctx.shape, ctx.state_shape = tuple(out.shape), tuple(leaving.shape)
            return out, leaving

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out, grad_leaving):
            plan = ctx.plan
            need_x, need_state, *need = ctx.needs_input_grad[2:]
            count = len(need)
            if ctx.with_frames:
                x, *rest = ctx.saved_tensors
                state = rest.pop() if ctx.has_state else None
                frames, out, kept = rest[:count], rest[count], rest[count + 1:]
            else:
                x, frames, out, kept, state = None, ctx.saved_tensors, None, None, None
            sections = [frames[i:i + 5] for i in range(0, count, 5)]
            device = (grad_out if grad_out is not None else grad_leaving).device
            g = _plan_layout(plan, grad_out) if grad_out is not None else torch.zeros(ctx.shape, dtype=torch.float32, device=device)
            if grad_leaving is not None:
                grad_leaving = grad_leaving.to(torch.float32).contiguous()
            grads = [tuple(torch.empty_like(t) for t in s) for s in sections] if ctx.with_frames else None
            with torch.cuda.device(device):
                gin, grads, gstate = plan.backward_cascade_frames_stream(x, sections, ctx.hop, kept, out, g, None, grads, state, grad_leaving,
                                                                         None if need_state else False)
            given = [t for s in grads for t in s] if grads is not None else [None] * count
            return (None, None, gin if need_x else None, gstate if need_state else None) + tuple(t if wanted else None for t, wanted in zip(given, need))

    _var2_cascade_frames_stream_function = Var2CascadeFramesStreamFunction
    return _var2_cascade_frames_stream_function


def _cascade_frames_function():
    """the torch.autograd.Function behind Var2Plan.apply_cascade_frames: (plan, hop, x, then the 5 K frame tensors)"""
    global _var2_cascade_frames_function
    if _var2_cascade_frames_function is not None:
        return _var2_cascade_frames_function
    import torch

    class Var2CascadeFramesFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, hop, x, *frames):
            ctx.plan, ctx.hop = plan, hop
            sections = [frames[i:i + 5] for i in range(0, len(frames), 5)]
            ctx.with_frames = any(ctx.needs_input_grad[3:])
            with torch.cuda.device(x.device):
                if ctx.with_frames:
                    out, kept = plan.execute_cascade_frames(x, sections, hop, keep=True)
                    ctx.save_for_backward(x, *frames, out, *kept)
                else:      # the backward reads nothing of the forward
                    out = plan.execute_cascade_frames(x, sections, hop)
                    ctx.save_for_backward(*frames)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            plan = ctx.plan
            need_x, *need = ctx.needs_input_grad[2:]
            count = len(need)
            if ctx.with_frames:
                x, *rest = ctx.saved_tensors
                frames, out, kept = rest[:count], rest[count], rest[count + 1:]
            else:
                x, frames, out, kept = None, ctx.saved_tensors, None, None
            sections = [frames[i:i + 5] for i in range(0, count, 5)]
            g = _plan_layout(plan, grad_out)
            grads = [tuple(torch.empty_like(t) for t in s) for s in sections] if ctx.with_frames else None
            with torch.cuda.device(g.device):
                gin, grads = plan.backward_cascade_frames(x, sections, ctx.hop, kept, out, g, None, grads)
            given = [t for s in grads for t in s] if grads is not None else [None] * count
            return (None, None, gin if need_x else None) + tuple(t if wanted else None for t, wanted in zip(given, need))

    _var2_cascade_frames_function = Var2CascadeFramesFunction
    return _var2_cascade_frames_function


def _biquad_frames_function():
    """the torch.autograd.Function behind Var2Plan.apply_biquad_frames: (plan, hop, x, then the five frame tensors)"""
    global _var2_biquad_frames_function
    if _var2_biquad_frames_function is not None:
        return _var2_biquad_frames_function
    import torch

    class Var2BiquadFramesFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, hop, x, b0, b1, b2, a1, a2):
            ctx.plan, ctx.hop = plan, hop
            with torch.cuda.device(x.device):
                out = plan.execute_biquad_frames(x, (b0, b1, b2, a1, a2), hop)
            ctx.save_for_backward(x, b0, b1, b2, a1, a2, out)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            plan = ctx.plan
            x, *frames, out = ctx.saved_tensors
            need_x, *need = ctx.needs_input_grad[2:8]
            g = _plan_layout(plan, grad_out)
            grads = tuple(torch.empty_like(t) for t in frames) if any(need) else None
            with torch.cuda.device(g.device):
                gin, grads = plan.backward_biquad_frames(x, frames, ctx.hop, out, g, None, grads)
            grads = grads if grads is not None else (None,) * 5
            return (None, None, gin if need_x else None) + tuple(t if wanted else None for t, wanted in zip(grads, need))

    _var2_biquad_frames_function = Var2BiquadFramesFunction
    return _var2_biquad_frames_function


def _biquad_function():
    """the torch.autograd.Function behind Var2Plan.apply_biquad"""
    global _var2_biquad_function
    if _var2_biquad_function is not None:
        return _var2_biquad_function
    import torch

    class Var2BiquadFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, x, b0, b1, b2, a1, a2):
            ctx.plan = plan
            with torch.cuda.device(x.device):
                out = plan.execute_biquad(x, b0, b1, b2, a1, a2)
            ctx.save_for_backward(x, b0, b1, b2, a1, a2, out)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            plan = ctx.plan
            *inputs, out = ctx.saved_tensors
            need_x, *need = ctx.needs_input_grad[1:7]
            g = _plan_layout(plan, grad_out)
            grads = tuple(plan._like(g) for _ in range(5)) if any(need) else None
            with torch.cuda.device(g.device):
                gin, grads = plan.backward_biquad(*inputs, out, g, None, grads)
            grads = grads if grads is not None else (None,) * 5
            return (None, gin if need_x else None) + tuple(t if wanted else None for t, wanted in zip(grads, need))

    _var2_biquad_function = Var2BiquadFunction
    return _var2_biquad_function


def _function():
    """the torch.autograd.Function behind Var2Plan.apply (torch is imported when it is first needed)"""
    global _var2_function
    if _var2_function is not None:
        return _var2_function
    import torch

    class Var2ScanFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, plan, x, a1, a2):
            ctx.plan = plan
            with torch.cuda.device(x.device):
                out = plan.execute(x, a1, a2)
            ctx.save_for_backward(a1, a2, out)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad_out):
            plan = ctx.plan
            a1, a2, out = ctx.saved_tensors
            need_x, need_1, need_2 = ctx.needs_input_grad[1:4]
            g = _plan_layout(plan, grad_out)
            g1 = plan._like(g) if need_1 or need_2 else None
            g2 = plan._like(g) if need_1 or need_2 else None
            with torch.cuda.device(g.device):
                gin, g1, g2 = plan.backward(a1, a2, out, g, None, g1, g2)
            return None, gin if need_x else None, g1 if need_1 else None, g2 if need_2 else None

    _var2_function = Var2ScanFunction
    return _var2_function


def _plan_layout(plan, t):
    """`t` as the plan takes a signal: f32, dense rows `stride` apart, 16-byte aligned (a copy only where it is not)"""
    import torch
    t = t.to(torch.float32)
    ok = t.stride(-1) == 1 and (t.dim() == 1 or plan.lines == 1 and t.is_contiguous() or plan.lines > 1 and t.stride(0) == plan.stride)
    if ok and t.data_ptr() % 16 == 0:
        return t
    fresh = plan._like(t)
    fresh.copy_(t)
    return fresh


_plans: Dict[tuple, Var2Plan] = {}


def allpole_scan(x, a1, a2, causal: bool = True):
    """y[n] = x[n] - a1[n] y[n-1] - a2[n] y[n-2]  (causal=False: y[n+1], y[n+2]) on device tensors of one shape, (N,) or (L, N),
    f32; every line has its own coefficients.  Differentiable in all three.  Plans are cached by length, lines, direction and
    device; calls that share a plan are ordered by the caller (one stream).  The library takes lengths that are multiples of 4:
    any other length is padded up to the next one with zeros in x, a1 and a2 -- behind the end for a causal scan, before the
    start for an anticausal one: the recurrence reaches the padding last and the masked coefficients stay where they were, so the
    N real samples are what an unpadded scan gives -- and the result is sliced back.  The padding costs one copy of every signal."""
    import torch
    if x.dim() not in (1, 2) or tuple(a1.shape) != tuple(x.shape) or tuple(a2.shape) != tuple(x.shape):
        raise ValueError(f"x, a1 and a2 must share one shape (N,) or (L, N), got {tuple(x.shape)}, {tuple(a1.shape)}, {tuple(a2.shape)}")
    n = int(x.shape[-1])
    lines = 1 if x.dim() == 1 else int(x.shape[0])
    pad = -n % 4
    device = x.device.index if x.device.index is not None else torch.cuda.current_device()
    key = (n + pad, lines, bool(causal), device)
    plan = _plans.get(key)
    if plan is None:
        plan = _plans[key] = Var2Plan(n + pad, lines=lines, causal=causal, device=device)
    if pad:
        where = (0, pad) if causal else (pad, 0)
        x, a1, a2 = (torch.nn.functional.pad(t, where) for t in (x, a1, a2))
    out = plan.apply(*(_plan_layout(plan, t) for t in (x, a1, a2)))
    if pad:
        out = out[..., :n] if causal else out[..., pad:]
    return out


def biquad_scan(x, b0, b1, b2, a1, a2, causal: bool = True):
    """The direct-form-I section with time-varying coefficients,
        v[n] = b0[n] x[n] + b1[n] x[n-1] + b2[n] x[n-2]        y[n] = v[n] - a1[n] y[n-1] - a2[n] y[n-2]
    (causal=False: the samples after n) on device tensors of one shape, (N,) or (L, N), f32; every line has its own coefficients.
    Differentiable in all six.  It shares allpole_scan's plan cache and its padding rule: a length that is no multiple of 4 is
    padded with zeros in all six signals, behind the end for a causal section, before the start for an anticausal one."""
    import torch
    signals = (x, b0, b1, b2, a1, a2)
    if x.dim() not in (1, 2) or any(tuple(t.shape) != tuple(x.shape) for t in signals):
        raise ValueError(f"x, b0, b1, b2, a1 and a2 must share one shape (N,) or (L, N), got {[tuple(t.shape) for t in signals]}")
    n = int(x.shape[-1])
    lines = 1 if x.dim() == 1 else int(x.shape[0])
    pad = -n % 4
    device = x.device.index if x.device.index is not None else torch.cuda.current_device()
    key = (n + pad, lines, bool(causal), device)
    plan = _plans.get(key)
    if plan is None:
        plan = _plans[key] = Var2Plan(n + pad, lines=lines, causal=causal, device=device)
    if pad:
        where = (0, pad) if causal else (pad, 0)
        signals = tuple(torch.nn.functional.pad(t, where) for t in signals)
    out = plan.apply_biquad(*(_plan_layout(plan, t) for t in signals))
    if pad:
        out = out[..., :n] if causal else out[..., pad:]
    return out


def biquad_cascade(x, sections: Sequence, causal: bool = True, keep: bool = False):
    """K direct-form-I sections with time-varying coefficients, one behind the other in one direction, in 2 K + 1 launches:
    `sections` is a sequence of K tuples (b0, b1, b2, a1, a2), 1 <= K <= 16, every signal a device tensor shaped like x, (N,) or
    (L, N), f32.  Differentiable in x and all 5 K coefficient signals; autograd keeps no signal between the sections.
    keep=True, the route for training: the values are the same bit for bit; where a coefficient signal requires a gradient the
    forward keeps every section's result (K - 1 more signals saved for the backward) and the backward reruns nothing
    (Var2Plan.backward_cascade_kept: 3 K + 1 launches for 6 K - 1).  The gradients of the two routes agree to rounding.  It shares
    biquad_scan's plan cache and padding rule: a length that is no multiple of 4 is padded with zeros in every signal, behind the
    end for causal sections, before the start for anticausal ones (a padded section maps zeros to zeros and the recurrence
    reaches the padding last, so the real samples are the unpadded cascade's)."""
    import torch
    sections = [tuple(s) for s in sections]
    if not 1 <= len(sections) <= capi.RF_VAR2_MAX_SECTIONS or any(len(s) != 5 for s in sections):
        raise ValueError(f"sections: 1..{capi.RF_VAR2_MAX_SECTIONS} tuples (b0, b1, b2, a1, a2)")
    signals = (x,) + tuple(t for s in sections for t in s)
    if x.dim() not in (1, 2) or any(tuple(t.shape) != tuple(x.shape) for t in signals):
        raise ValueError(f"x and every coefficient signal must share one shape (N,) or (L, N), got {sorted({tuple(t.shape) for t in signals})}")
    n = int(x.shape[-1])
    lines = 1 if x.dim() == 1 else int(x.shape[0])
    pad = -n % 4
    device = x.device.index if x.device.index is not None else torch.cuda.current_device()
    key = (n + pad, lines, bool(causal), device)
    plan = _plans.get(key)
    if plan is None:
        plan = _plans[key] = Var2Plan(n + pad, lines=lines, causal=causal, device=device)
    if pad:
        where = (0, pad) if causal else (pad, 0)
        signals = tuple(torch.nn.functional.pad(t, where) for t in signals)
    signals = [_plan_layout(plan, t) for t in signals]
    out = plan.apply_cascade(signals[0], [signals[1 + 5 * k:6 + 5 * k] for k in range(len(sections))], keep=keep)
    if pad:
        out = out[..., :n] if causal else out[..., pad:]
    return out


def frames_count(length: int, hop: int) -> int:
    """rf_var2_frames_count: the frames per coefficient and line that `length` samples take at one frame every `hop` samples,
    ceil(length / hop) + 1 -- frame j sits at sample j * hop and the last interval has both its ends.  hop: a power of two,
    64..65536 (anything else raises ValueError)."""
    count = int(capi.lib().rf_var2_frames_count(int(length), int(hop))) if 1 <= int(length) <= 2 ** 30 else 0
    if count == 0:
        raise ValueError(f"hop must be a power of two in 64..65536 and length 1..2**30 (got hop {hop}, length {length})")
    return count


def expand_frames(frames, hop: int, length: int, out=None, stream=None):
    """rf_var2_expand_frames: the coefficient signal the frames kernels form in registers, at audio rate.  frames: a device tensor
    (F,) or (L, F), f32, F = frames_count(length, hop), dense rows (a [:, :F] view of a wider buffer is taken as it is); the
    result is (length,) or (L, length):  c[j * hop + k] = fma(k / hop, c[j+1] - c[j], c[j]).  out: a tensor to be written, rows a
    multiple of 4 samples apart (then length is a multiple of 4 too); None allocates it."""
    import torch
    count = frames_count(length, hop)
    if frames.dim() not in (1, 2) or int(frames.shape[-1]) != count:
        raise ValueError(f"frames: shape {tuple(frames.shape)}, {length} samples at hop {hop} take (..., {count})")
    if frames.dtype != torch.float32 or not frames.is_cuda or frames.stride(-1) != 1:
        raise ValueError("frames: a float32 device tensor with dense rows")
    lines = 1 if frames.dim() == 1 else int(frames.shape[0])
    frame_stride = int(frames.stride(0)) if frames.dim() == 2 and lines > 1 else count
    padded = length + (-length % 4)
    if out is None:
        result = torch.empty(frames.shape[:-1] + (padded,), dtype=torch.float32, device=frames.device)
    else:
        result = out
        if tuple(out.shape) != tuple(frames.shape[:-1]) + (length,) or out.dtype != torch.float32 or not out.is_cuda or out.stride(-1) != 1 or padded != length:
            raise ValueError(f"out: a float32 device tensor {tuple(frames.shape[:-1]) + (length,)} with dense rows, length a multiple of 4")
    stride = int(result.stride(0)) if result.dim() == 2 and lines > 1 else padded
    with torch.cuda.device(frames.device):
        s = _PlanHandle._stream(stream)
        capi.check(capi.lib().rf_var2_expand_frames(ctypes.c_void_p(frames.data_ptr()), int(hop), count, frame_stride, padded, lines, stride,
                                                    ctypes.c_void_p(result.data_ptr()), s))
    return result if out is not None else result[..., :length]


def biquad_scan_frames(x, b0, b1, b2, a1, a2, hop: int, causal: bool = True):
    """biquad_scan with the five coefficients at a control rate: x is (N,) or (L, N), every coefficient (F,) or (L, F) with
    F = frames_count(N, hop), frame j at sample j * hop and linear interpolation between two frames (expand_frames), by absolute
    position for either direction.  hop: a power of two, 64..65536.  The kernels read the frames and interpolate in registers: no
    audio-rate coefficient signal exists, forward or backward.  Differentiable in x and all five frame tensors -- the frame
    gradients are the per-sample gradients contracted in f64; x, the frames and the result are saved, no double backward.
    b = (1, 0, 0) frames is the all-pole scan.  Frames must be finite.  It shares biquad_scan's plan cache; a length that is no
    multiple of 4 is padded with zeros in x behind the END for either direction (hop is a multiple of 4: F does not change, and
    zero input on zero state stays zero)."""
    import torch
    frames = (b0, b1, b2, a1, a2)
    n = int(x.shape[-1])
    count = frames_count(n, hop)
    shape = tuple(x.shape[:-1]) + (count,)
    if x.dim() not in (1, 2) or any(tuple(t.shape) != shape for t in frames):
        raise ValueError(f"x is (N,) or (L, N) and every frame tensor {shape} at hop {hop}, got {tuple(x.shape)} and {[tuple(t.shape) for t in frames]}")
    lines = 1 if x.dim() == 1 else int(x.shape[0])
    pad = -n % 4
    device = x.device.index if x.device.index is not None else torch.cuda.current_device()
    key = (n + pad, lines, bool(causal), device)
    plan = _plans.get(key)
    if plan is None:
        plan = _plans[key] = Var2Plan(n + pad, lines=lines, causal=causal, device=device)
    if pad:
        x = torch.nn.functional.pad(x, (0, pad))
    out = plan.apply_biquad_frames(_plan_layout(plan, x), tuple(t.to(torch.float32).contiguous() for t in frames), hop)
    return out[..., :n] if pad else out


def biquad_cascade_frames(x, sections: Sequence, hop: int, causal: bool = True):
    """biquad_cascade with every section's five coefficients at a control rate: K sections, 1 <= K <= 16, one behind the other
    in one direction, in 2 K + 1 launches that read no coefficient signal.  x is (N,) or (L, N); `sections` is K tuples
    (b0, b1, b2, a1, a2) of frame tensors (F,) or (L, F), F = frames_count(N, hop), frame j at sample j * hop, linear
    interpolation between two frames by absolute position for either direction; one hop, a power of two in 64..65536, serves
    all sections.  Differentiable in x and all 5 K frame tensors.  Where a frame tensor requires a gradient the forward keeps
    every section's result (x, the frames, the result and K - 1 signals are saved) and the backward reruns nothing; where only
    x does, the frames alone are saved.  The values are biquad_cascade's on expand_frames of every coefficient, bit for bit.
    It shares biquad_scan's plan cache and pads as biquad_scan_frames does: a length that is no multiple of 4 gets zeros in x
    behind the END for either direction."""
    import torch
    sections = [tuple(s) for s in sections]
    if not 1 <= len(sections) <= capi.RF_VAR2_MAX_SECTIONS or any(len(s) != 5 for s in sections):
        raise ValueError(f"sections: 1..{capi.RF_VAR2_MAX_SECTIONS} tuples (b0, b1, b2, a1, a2) of frame tensors")
    n = int(x.shape[-1])
    count = frames_count(n, hop)
    shape = tuple(x.shape[:-1]) + (count,)
    if x.dim() not in (1, 2) or any(tuple(t.shape) != shape for s in sections for t in s):
        raise ValueError(f"x is (N,) or (L, N) and every frame tensor {shape} at hop {hop}, got {tuple(x.shape)} and "
                         f"{sorted({tuple(t.shape) for s in sections for t in s})}")
    lines = 1 if x.dim() == 1 else int(x.shape[0])
    pad = -n % 4
    device = x.device.index if x.device.index is not None else torch.cuda.current_device()
    key = (n + pad, lines, bool(causal), device)
    plan = _plans.get(key)
    if plan is None:
        plan = _plans[key] = Var2Plan(n + pad, lines=lines, causal=causal, device=device)
    if pad:
        x = torch.nn.functional.pad(x, (0, pad))
    out = plan.apply_cascade_frames(_plan_layout(plan, x), [tuple(t.to(torch.float32).contiguous() for t in s) for s in sections], hop)
    return out[..., :n] if pad else out


def biquad_cascade_frames_stream(x, sections: Sequence, hop: int, state=None, causal: bool = True):
    """biquad_cascade_frames on one chunk of a longer signal: (y, state).  `state` is what the call on the chunk before returned
    (None: silence), (K + 1, 2) for x of shape (N,) or (L, K + 1, 2) for (L, N): pair 0 the two last samples of the input so far,
    pair k + 1 those of section k's result, the nearest first.  N must be a multiple of 4 -- padding would corrupt the state that
    leaves -- so a ragged length raises ValueError.  `sections` holds the chunk's frames, F = frames_count(N, hop) per tensor: for
    a chunk that starts at sample s of the whole signal, s a multiple of hop, the slice [..., s // hop : s // hop + F] of the
    whole signal's frames.  causal=False: the chunks are fed last to first and the state is (x[n], x[n+1]), ...  Chunks chained
    this way give what one biquad_cascade_frames call on the whole signal gives, to rounding.  Differentiable in x, in all 5 K
    frame tensors and in `state`, and a gradient flows into the returned state: a loss on a chain of chunks reaches every chunk
    (detach the state for truncated back-propagation through time).  It shares biquad_scan's plan cache."""
    import torch
    sections = [tuple(s) for s in sections]
    K = len(sections)
    if not 1 <= K <= capi.RF_VAR2_MAX_SECTIONS or any(len(s) != 5 for s in sections):
        raise ValueError(f"sections: 1..{capi.RF_VAR2_MAX_SECTIONS} tuples (b0, b1, b2, a1, a2) of frame tensors")
    n = int(x.shape[-1])
    if n < 4 or n % 4 != 0:
        raise ValueError(f"a chunk's length must be a positive multiple of 4 (padding would corrupt the state that leaves), got {n}")
    count = frames_count(n, hop)
    shape = tuple(x.shape[:-1]) + (count,)
    if x.dim() not in (1, 2) or any(tuple(t.shape) != shape for s in sections for t in s):
        raise ValueError(f"x is (N,) or (L, N) and every frame tensor {shape} at hop {hop}, got {tuple(x.shape)} and "
                         f"{sorted({tuple(t.shape) for s in sections for t in s})}")
    lines = 1 if x.dim() == 1 else int(x.shape[0])
    if state is not None and tuple(state.shape) != tuple(x.shape[:-1]) + (K + 1, 2):
        raise ValueError(f"state: shape {tuple(state.shape)}, x of shape {tuple(x.shape)} and {K} sections take {tuple(x.shape[:-1]) + (K + 1, 2)}")
    device = x.device.index if x.device.index is not None else torch.cuda.current_device()
    key = (n, lines, bool(causal), device)
    plan = _plans.get(key)
    if plan is None:
        plan = _plans[key] = Var2Plan(n, lines=lines, causal=causal, device=device)
    if state is not None:
        state = state.to(torch.float32).contiguous()
    out, state = plan.apply_cascade_frames_stream(_plan_layout(plan, x), [tuple(t.to(torch.float32).contiguous() for t in s) for s in sections], hop, state)
    return out, state.reshape(tuple(x.shape[:-1]) + (K + 1, 2))


class BiquadCascadeStream:
    """A cascade of K sections on control-rate frames that remembers where it stopped: push(x, sections) filters the next chunk
    and returns its result; chunks pushed one after the other give what biquad_cascade_frames gives on their concatenation, to
    rounding.  x is (N,) (lines == 1) or (lines, N), N a multiple of 4; `sections` the chunk's frames as
    biquad_cascade_frames_stream takes them; causal=False: push the chunks last to first.  The state is detached and lives in two
    buffers that swap roles: one enters a call while the other receives what leaves it.  reset() returns to silence; between two
    resets every chunk has one device and one layout ((N,) or (lines, N)): anything else raises."""

    def __init__(self, K: int, hop: int, lines: int = 1, causal: bool = True):
        if not 1 <= int(K) <= capi.RF_VAR2_MAX_SECTIONS:
            raise ValueError(f"K: 1..{capi.RF_VAR2_MAX_SECTIONS} sections")
        frames_count(4, hop)      # (refuses the hop)
        self.K, self.hop, self.lines, self.causal = int(K), int(hop), int(lines), bool(causal)
        self._buffers = None
        self._entering = None      # the index of the buffer that enters the next push; None: silence

    def reset(self) -> None:
        self._entering = None

    @property
    def state(self):
        """the state that enters the next push (a view of the stream's buffer; None: silence)"""
        return None if self._entering is None else self._buffers[self._entering]

    def push(self, x, sections: Sequence):
        import torch
        if x.dim() not in (1, 2) or (x.dim() == 1 and self.lines != 1) or (x.dim() == 2 and int(x.shape[0]) != self.lines) or len(sections) != self.K:
            raise ValueError(f"x: ({self.lines}, N) and {self.K} sections, got {tuple(x.shape)} and {len(sections)}")
        shape = (self.K + 1, 2) if x.dim() == 1 else (self.lines, self.K + 1, 2)
        if self._entering is not None and (self._buffers[0].device != x.device or tuple(self._buffers[0].shape) != shape):
            # a stream that went on from silence here would be wrong without a word
            raise ValueError(f"x: the stream holds a state of shape {tuple(self._buffers[0].shape)} on {self._buffers[0].device}, got x of shape "
                             f"{tuple(x.shape)} on {x.device}; reset() first")
        if self._buffers is None or self._buffers[0].device != x.device or tuple(self._buffers[0].shape) != shape:
            self._buffers = [torch.empty(shape, dtype=torch.float32, device=x.device) for _ in range(2)]
        n = int(x.shape[-1])
        if n < 4 or n % 4 != 0:
            raise ValueError(f"a chunk's length must be a positive multiple of 4, got {n}")
        device = x.device.index if x.device.index is not None else torch.cuda.current_device()
        key = (n, self.lines, self.causal, device)
        plan = _plans.get(key)
        if plan is None:
            plan = _plans[key] = Var2Plan(n, lines=self.lines, causal=self.causal, device=device)
        leaving = 0 if self._entering is None else 1 - self._entering
        with torch.no_grad(), torch.cuda.device(x.device):
            frames = [tuple(t.detach().to(torch.float32).contiguous() for t in s) for s in sections]
            out, _ = plan.execute_cascade_frames_stream(_plan_layout(plan, x.detach()), frames, self.hop, self.state, state_out=self._buffers[leaving])
        self._entering = leaving
        return out
