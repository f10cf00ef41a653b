"""Guarded planes and statelessness checks (a plain module: no fixtures).  tests/test_gpu_footprint.py drives the HIP paths
with it, tests/test_footprint_host.py drives it with CPU tensors and stand-in executes that commit one defect at a time.

Two questions the parity tests do not ask:

  * did an execute stay inside its planes?  Planes lie back to back in ONE allocation per role with guards before, between and
    behind them.  Output guards hold 0xA5 and must be unchanged afterwards; input guards hold 0xFF (a NaN in f32, f64, f16 and
    bf16), so a load past a plane that is masked by `0 *` instead of a select turns the result into NaN, which the oracle
    assertion refuses; integer planes run a second time with 0x00 guards and the two results must be bit-identical.  An
    out-of-place run must leave every byte of the input allocation as it was.
  * does a plan keep state across steps, or read scratch nothing wrote in this step?  three_steps: A, poison, A on one plan and
    one stream -- the third result bit-identical to the first.  poisoned_scratch: every scratch buffer of a NEW plan filled
    with 0xFF before its first execute -- bit-identical to an unfilled plan's result.

Bit identity rests on the kernels being deterministic from run to run (no floating-point atomics in the sources)."""
from __future__ import annotations

import numpy as np

OUT_FILL = 0xA5          # output guards
IN_FILL = 0xFF           # input guards: NaN in every float type
IN_FILL_ZERO = 0x00      # integer / uint8 planes: the second run
MIN_GUARD_ELEMS = 4096
ALIGN = 256              # guards are multiples of this many bytes, planes start on such a boundary (before lead_elems)


def torch_dtype(dtype):
    """the torch type of a numpy or torch pixel type"""
    import torch
    if isinstance(dtype, torch.dtype):
        return dtype
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
            np.dtype(np.int16): torch.int16, np.dtype(np.float16): torch.float16, np.dtype(np.uint8): torch.uint8}[np.dtype(dtype)]


def _round_up(n, m):
    return (n + m - 1) // m * m


def layout(shape, itemsize, planes, guard_bytes=0, lead_elems=0):
    """Byte layout of one guarded allocation: (total bytes, guard bytes, [plane offsets], plane bytes).  The guard is at least
    MIN_GUARD_ELEMS elements and `guard_bytes`, rounded up to ALIGN; plane i starts at guard + i * (round_up(plane, ALIGN) +
    guard) + lead_elems * itemsize, so without a lead every plane is ALIGN-byte (hence 16-byte) aligned, and a lead shifts all
    planes by whole elements.  Everything outside the planes is guard: at least `guard` bytes on every side of every plane."""
    plane_bytes = int(np.prod(shape, dtype=np.int64)) * itemsize
    guard = _round_up(max(int(guard_bytes), MIN_GUARD_ELEMS * itemsize), ALIGN)
    lead = int(lead_elems) * itemsize
    if not 0 <= lead < guard - ALIGN + 1:
        raise ValueError("lead_elems must leave most of the guard in place")
    pitch = _round_up(plane_bytes, ALIGN) + guard
    # (one more guard behind the last plane's pitch, so a lead never shortens the last guard below `guard`)
    offsets = [guard + i * pitch + lead for i in range(planes)]
    total = guard + planes * pitch + guard
    return total, guard, offsets, plane_bytes


class Guarded:
    """One allocation of `planes` planes with guards.  views: the planes, contiguous, of exactly `shape`."""

    def __init__(self, shape, dtype, planes, guard_bytes=0, lead_elems=0, fill=OUT_FILL, device="cuda"):
        import torch
        self.dtype = torch_dtype(dtype)
        self.shape = tuple(int(s) for s in shape)
        self.fill = int(fill)
        itemsize = torch.empty(0, dtype=self.dtype).element_size()
        self.total, self.guard, self.offsets, self.plane_bytes = layout(self.shape, itemsize, planes, guard_bytes, lead_elems)
        self.raw = torch.full((self.total,), self.fill, dtype=torch.uint8, device=device)
        if self.raw.data_ptr() % 16 != 0:       # (torch's allocators give 64 bytes on the host, 512 on the device)
            raise RuntimeError("allocation is not 16-byte aligned")
        self.views = [self.raw[o:o + self.plane_bytes].view(self.dtype).view(self.shape) for o in self.offsets]
        self._snapshot = None

    def guard_ranges(self):
        """[(begin, end)] of the guard bytes, in order"""
        edges = [0]
        for o in self.offsets:
            edges += [o, o + self.plane_bytes]
        edges.append(self.total)
        return [(edges[i], edges[i + 1]) for i in range(0, len(edges), 2)]

    def load(self, tensors):
        for v, t in zip(self.views, tensors):
            v.copy_(t)

    def snapshot(self):
        self._snapshot = self.raw.clone()

    def _where(self, byte):
        """a guard byte's position in words: which plane it is nearest to"""
        for i, o in enumerate(self.offsets):
            if byte < o:
                return f"{o - byte} bytes before plane {i}"
            if byte < o + self.plane_bytes:
                return f"byte {byte - o} of plane {i}"
        return f"{byte - (self.offsets[-1] + self.plane_bytes)} bytes behind the last plane"

    def check_guards(self, what="output"):
        """every guard byte still holds the fill"""
        for a, b in self.guard_ranges():
            bad = self.raw[a:b] != self.fill
            if bool(bad.any()):
                first = a + int(bad.nonzero()[0])
                raise AssertionError(f"{what} guard written: {int(bad.sum())} bytes, the first one {self._where(first)} "
                                     f"(value {int(self.raw[first]):#04x}, guards hold {self.fill:#04x})")

    def check_unchanged(self, what="input"):
        """every byte of the allocation is what snapshot() saw, planes and guards alike"""
        import torch
        if self._snapshot is None:
            raise RuntimeError("no snapshot")
        if not torch.equal(self.raw, self._snapshot):
            bad = self.raw != self._snapshot
            first = int(bad.nonzero()[0])
            raise AssertionError(f"{what} allocation written: {int(bad.sum())} bytes, the first one {self._where(first)}")


def guarded_planes(shape, dtype, planes, guard_bytes=0, lead_elems=0, fill=OUT_FILL, device="cuda"):
    """(plane views, checker) of one guarded allocation; the checker is the Guarded object (check_guards, snapshot,
    check_unchanged)."""
    g = Guarded(shape, dtype, planes, guard_bytes, lead_elems, fill, device)
    return g.views, g


def _sync(device):
    if str(device).startswith("cuda"):
        import torch
        torch.cuda.synchronize()


def bits_equal(a, b):
    """bit identity of two tensors of one type and shape (NaNs compare by their bits)"""
    import torch
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def assert_bits_equal(a_list, b_list, what):
    for i, (a, b) in enumerate(zip(a_list, b_list)):
        if not bits_equal(a, b):
            import torch
            d = a.contiguous().reshape(-1).view(torch.uint8) != b.contiguous().reshape(-1).view(torch.uint8)
            raise AssertionError(f"{what}: plane {i} differs in {int(d.sum())} bytes, the first one at byte {int(d.nonzero()[0])}")


def guarded_execute(execute, shape, in_dtype, out_dtype, inputs, inplace=False, in_fill=IN_FILL, lead_in=0, lead_out=0,
                    guard_bytes=0, device="cuda"):
    """One execute on guarded planes.  `execute(ins, outs)` runs the plan (or a stand-in); `inputs` are tensors of `in_dtype`
    copied into the input planes.  Out of place: the output allocation's guards (0xA5) must be unchanged and so must every byte
    of the input allocation (guards `in_fill`).  In place: input and output are ONE allocation with `in_fill` guards, which
    must be unchanged.  Returns the outputs, copied to the host."""
    planes = len(inputs)
    if inplace:
        views, g = guarded_planes(shape, out_dtype, planes, guard_bytes, lead_out, in_fill, device)
        g.load(inputs)
        execute(views, views)
        _sync(device)
        g.check_guards("in-place")
        return [v.clone().cpu() for v in views]
    ins, gi = guarded_planes(shape, in_dtype, planes, guard_bytes, lead_in, in_fill, device)
    outs, go = guarded_planes(shape, out_dtype, planes, guard_bytes, lead_out, OUT_FILL, device)
    gi.load(inputs)
    gi.snapshot()
    execute(ins, outs)
    _sync(device)
    go.check_guards("output")
    gi.check_unchanged("input")
    return [v.clone().cpu() for v in outs]


def _fresh(tensors, device):
    return [t.to(device).clone().contiguous() for t in tensors]


def three_steps(plan, A, poison, out_dtype=None, inplace=False, execute=None, device="cuda"):
    """A -> r1, poison, A -> r3 on one plan and one stream; the plan must still hold one instance and r3 must be bit-identical
    to r1.  `execute(ins, outs)` defaults to plan.execute; A and poison are lists of tensors (any device).  Returns r1 on the
    host."""
    import torch
    run = execute or (lambda ins, outs: plan.execute(ins, outs))
    tdt = torch_dtype(out_dtype) if out_dtype is not None else A[0].dtype

    def step(src):
        ins = _fresh(src, device)
        outs = ins if inplace else [torch.empty(t.shape, dtype=tdt, device=device) for t in ins]
        run(ins, outs)
        _sync(device)
        return [o.cpu() for o in outs]
    r1 = step(A)
    step(poison)
    r3 = step(A)
    assert plan.num_instances == 1, f"the plan built {plan.num_instances} instances on one stream"
    assert_bits_equal(r3, r1, "step 3 against step 1 (state kept across steps)")
    return r1


def poisoned_scratch(plan, A, r1, out_dtype=None, inplace=False, execute=None, byte=0xFF, device="cuda"):
    """`plan` is NEW (never executed): every scratch buffer is filled with `byte`, then A runs; the result must be bit-identical
    to r1, the result of an unfilled plan.  Returns how many buffers were filled."""
    import torch
    run = execute or (lambda ins, outs: plan.execute(ins, outs))
    tdt = torch_dtype(out_dtype) if out_dtype is not None else A[0].dtype
    filled = 0
    for index, kind, _ in plan.debug_buffers():
        if kind == "scratch":
            plan.debug_fill(index, byte)
            filled += 1
    ins = _fresh(A, device)
    outs = ins if inplace else [torch.empty(t.shape, dtype=tdt, device=device) for t in ins]
    run(ins, outs)
    _sync(device)
    assert_bits_equal([o.cpu() for o in outs], r1, "poisoned scratch against a fresh plan (scratch read before it is written)")
    return filled


TOL = 1e-4
HALF_EPS = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}       # half an ulp of the one rounding (tests/test_gpu_half_pixels.py)


def assert_oracle(got, want, kind, scale=None):
    """The suite's own assertion, unchanged.  got: a host tensor; want: the f64 oracle's result (of the widened input for the
    16-bit types; rc.pointwise_want's, with its scale, for plans with an epilogue).  Floats: rc.rel_err < 1e-4 (+ 2^-11 for
    f16, 2^-8 for bf16) -- a NaN anywhere fails it.  Integers: bit-exact."""
    import ref_cases as rc
    if kind in ("i32", "i16"):
        np.testing.assert_array_equal(got.numpy(), want)
        return 0.0
    out = got.float().numpy() if kind in HALF_EPS else got.numpy()
    err = rc.rel_err(out, want, scale=scale)
    bar = TOL + HALF_EPS.get(kind, 0.0)
    assert err < bar, f"rel err {err} against {bar}"
    return err


def nan_like(t):
    """the poison of float planes: an all-NaN image"""
    import torch
    return torch.full(t.shape, float("nan"), dtype=t.dtype)
