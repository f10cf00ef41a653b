"""tests/guarded.py on the host: the checker must fail when a kernel is wrong.  A stand-in "execute" on CPU tensors (the oracle
itself, so the clean run passes the oracle assertion) commits one defect at a time; every defect must be caught.  Also the
layout arithmetic, rf_plan_debug_buffer_kind / rf_plan_debug_fill on host-only plans, and every row of
tests/test_gpu_footprint.py built as a host-only plan: path and tiles are the ones the row is meant for."""
import numpy as np
import pytest
import torch

import guarded
import oracle
import ref_cases as rc
import test_gpu_footprint as fp
from recfilter_amd import capi

SHAPE = (12, 20)
SCANS = [(0, True, [0.5, 0.5]), (1, False, [0.6, 0.4])]


def _inputs(planes=2, dtype=np.float32):
    return [torch.from_numpy(rc.random_image(SHAPE, dtype, 40 + p)) for p in range(planes)]


def _filter(t):
    if t.dtype in (torch.int32, torch.int16):
        return torch.from_numpy(np.asarray(oracle.apply_filter(t.numpy(), [(0, True, [1.0, 1.0])], False)).astype(t.numpy().dtype))
    return torch.from_numpy(oracle.apply_filter(t.numpy().astype(np.float64), SCANS, False).astype(np.float32))


def _outside(view, elems):
    """one element `elems` elements behind the end of a plane (negative: before its start), through the plane's storage"""
    at = view.storage_offset() + (view.numel() + elems - 1 if elems > 0 else elems)
    return view.as_strided((1,), (1,), at)


def clean(ins, outs):
    results = [_filter(i.clone()) for i in ins]       # (in place: ins are outs)
    for o, r in zip(outs, results):
        o.copy_(r)


def _defect(kind):
    def execute(ins, outs):
        if kind == "adds_zero_times_guard":
            results = [_filter(i.clone()) + 0.0 * _outside(i, 1) for i in ins]
            for o, r in zip(outs, results):
                o.copy_(r)
            return
        if kind == "adds_guard_value":       # (integer planes: what the 0x00-guard run is for)
            results = [_filter(i.clone()) + _outside(i, 1) for i in ins]
            for o, r in zip(outs, results):
                o.copy_(r)
            return
        clean(ins, outs)
        if kind == "past_last_plane":
            _outside(outs[-1], 1).fill_(1.0)
        elif kind == "before_first_plane":
            _outside(outs[0], -1).fill_(1.0)
        elif kind == "into_the_gap":
            _outside(outs[0], 100).fill_(1.0)
        elif kind == "writes_input":
            ins[0][0, 0] += 1.0
        elif kind == "past_the_lead":      # a store at the unshifted position of a plane that was given a lead
            _outside(outs[0], -3).fill_(1.0)
    return execute


def _run(execute, dtype=np.float32, kind="f32", inplace=False, in_fill=guarded.IN_FILL, lead_in=0, lead_out=0, planes=2):
    ins = _inputs(planes, dtype)
    got = guarded.guarded_execute(execute, SHAPE, dtype, dtype, ins, inplace=inplace, in_fill=in_fill, lead_in=lead_in, lead_out=lead_out,
                                  device="cpu")
    for g, i in zip(got, ins):
        want = oracle.apply_filter(i.numpy(), [(0, True, [1.0, 1.0])], False) if kind[0] == "i" else \
            oracle.apply_filter(i.numpy().astype(np.float64), SCANS, False)
        guarded.assert_oracle(g, want, kind)
    return got


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("lead", [0, 3])
def test_the_clean_stand_in_passes(inplace, lead):
    _run(clean, inplace=inplace, lead_in=lead, lead_out=lead)
    _run(clean, np.int32, "i32", inplace=inplace, lead_in=lead, lead_out=lead)


@pytest.mark.parametrize("defect", ["past_last_plane", "before_first_plane", "into_the_gap", "writes_input", "adds_zero_times_guard", "past_the_lead"])
def test_every_defect_is_caught_out_of_place(defect):
    with pytest.raises(AssertionError):
        _run(_defect(defect), lead_in=3, lead_out=3)


@pytest.mark.parametrize("defect", ["past_last_plane", "before_first_plane", "into_the_gap", "adds_zero_times_guard"])
def test_every_defect_is_caught_in_place(defect):
    with pytest.raises(AssertionError):
        _run(_defect(defect), inplace=True)


def test_integer_planes_need_both_guard_values():
    """an integer result that picks up a guard sample: exact with 0x00 guards, so only the pair of runs shows it"""
    zero = _run(_defect("adds_guard_value"), np.int32, "i32", in_fill=guarded.IN_FILL_ZERO)
    ins = _inputs(2, np.int32)
    ones = guarded.guarded_execute(_defect("adds_guard_value"), SHAPE, np.int32, np.int32, ins, in_fill=guarded.IN_FILL, device="cpu")
    with pytest.raises(AssertionError):
        guarded.assert_bits_equal(ones, zero, "0x00 input guards against 0xFF input guards")
    guarded.assert_bits_equal(_run(clean, np.int32, "i32", in_fill=guarded.IN_FILL_ZERO), _run(clean, np.int32, "i32"), "clean")


class StandInPlan:
    """what three_steps / poisoned_scratch need of a plan; `leak`: keeps 0 * (the last input's first sample) for the next
    step; `flip_on`: the execute (counted from 1) whose result differs in one bit; `reads_scratch`: adds 0 * scratch[0]"""

    def __init__(self, leak=False, flip_on=0, reads_scratch=False, instances=1):
        self.leak, self.flip_on, self.reads_scratch, self.num_instances = leak, flip_on, reads_scratch, instances
        self.calls, self.state = 0, torch.zeros(1)
        self.scratch, self.zeroed, self.table = torch.zeros(4), torch.zeros(4), torch.ones(4)

    def execute(self, ins, outs):
        self.calls += 1
        clean(ins, outs)
        if self.leak:
            for o in outs:
                o += self.state
            self.state = 0.0 * ins[0].reshape(-1)[:1].clone()
        if self.reads_scratch:
            outs[0] += 0.0 * self.scratch[0]
        if self.calls == self.flip_on:
            bits = outs[0].view(torch.int32).reshape(-1)
            bits[5] ^= 1
        return outs

    def debug_buffers(self):
        return [(0, "table", 16), (1, "zeroed", 16), (2, "scratch", 16)]

    def debug_fill(self, index, byte):
        assert index == 2, "only scratch may be filled"
        self.scratch.view(torch.uint8).fill_(byte)


@pytest.mark.parametrize("inplace", [False, True])
def test_three_steps(inplace):
    A = _inputs()
    poison = [guarded.nan_like(t) for t in A]
    r1 = guarded.three_steps(StandInPlan(), A, poison, inplace=inplace, device="cpu")
    assert guarded.bits_equal(r1[0], _filter(A[0]))
    with pytest.raises(AssertionError, match="step 3"):
        guarded.three_steps(StandInPlan(flip_on=3), A, poison, inplace=inplace, device="cpu")       # one bit
    with pytest.raises(AssertionError, match="step 3"):
        guarded.three_steps(StandInPlan(leak=True), A, poison, inplace=inplace, device="cpu")       # NaN kept from the poison step
    with pytest.raises(AssertionError, match="instances"):
        guarded.three_steps(StandInPlan(instances=2), A, poison, inplace=inplace, device="cpu")


def test_poisoned_scratch():
    A = _inputs()
    r1 = guarded.three_steps(StandInPlan(), A, [guarded.nan_like(t) for t in A], device="cpu")
    assert guarded.poisoned_scratch(StandInPlan(), A, r1, device="cpu") == 1
    with pytest.raises(AssertionError, match="scratch"):
        guarded.poisoned_scratch(StandInPlan(reads_scratch=True), A, r1, device="cpu")


def test_bits_equal_sees_one_bit_and_nan_payloads():
    a = torch.tensor([1.0, float("nan"), -0.0])
    assert guarded.bits_equal(a, a.clone())
    assert not guarded.bits_equal(a, torch.tensor([1.0, float("nan"), 0.0]))
    b = a.clone()
    b.view(torch.int32)[1] ^= 1
    assert not guarded.bits_equal(a, b)
    assert not guarded.bits_equal(a, a.double())


# ---- layout ----------------------------------------------------------------------------------------------------------------
ALL_TYPES = [torch.uint8, torch.int16, torch.float16, torch.bfloat16, torch.int32, torch.float32, torch.float64]


@pytest.mark.parametrize("dtype", ALL_TYPES, ids=[str(t).replace("torch.", "") for t in ALL_TYPES])
@pytest.mark.parametrize("shape", [(3, 1), (33, 21), (12345,), (5, 7, 9), (64, 256)])
@pytest.mark.parametrize("planes,lead", [(1, 0), (3, 0), (2, 1), (3, 4)])
def test_layout(dtype, shape, planes, lead):
    size = torch.empty(0, dtype=dtype).element_size()
    views, g = guarded.guarded_planes(shape, dtype, planes, lead_elems=lead, device="cpu")
    assert g.guard >= guarded.MIN_GUARD_ELEMS * size and g.guard % 256 == 0
    assert len(views) == planes
    base = g.raw.data_ptr()
    for v in views:
        assert tuple(v.shape) == tuple(shape) and v.is_contiguous() and v.dtype == dtype
        assert (v.data_ptr() - lead * size) % 16 == 0          # 16-byte aligned before the lead, shifted by whole elements
        assert (v.data_ptr() - base - lead * size) % 256 == 0
    # planes in order, at least one whole guard on every side, everything outside the planes is guard
    ranges = g.guard_ranges()
    assert len(ranges) == planes + 1 and ranges[0][0] == 0 and ranges[-1][1] == g.total
    for (a, b) in ranges:
        assert b - a >= g.guard
    covered = sum(b - a for a, b in ranges) + planes * g.plane_bytes
    assert covered == g.total
    for i, v in enumerate(views):
        assert v.data_ptr() - base == ranges[i][1] and ranges[i + 1][0] == ranges[i][1] + g.plane_bytes
    assert bool((g.raw == guarded.OUT_FILL).all())
    g.check_guards()
    views[-1].view(torch.uint8).reshape(-1)[-1] = 0          # the planes themselves are free
    g.check_guards()
    g.raw[ranges[-1][0]] = 0                                  # the byte behind the last plane is not
    with pytest.raises(AssertionError, match="behind the last plane"):
        g.check_guards()


def test_layout_guard_bytes_and_input_fill():
    total, guard, offsets, plane = guarded.layout((10, 10), 4, 2, guard_bytes=100_000)
    assert guard == 100_096 and plane == 400 and offsets == [guard, guard + 512 + guard] and total == 4 * guard + 2 * 512
    views, g = guarded.guarded_planes((10, 10), np.float32, 1, fill=guarded.IN_FILL, device="cpu")
    for dt in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
        assert bool(torch.isnan(g.raw[:64].view(dt)).all())                   # 0xFF is a NaN in every float type
    with pytest.raises(ValueError):
        guarded.layout((10, 10), 4, 1, lead_elems=4096)


# ---- the debug surface on host-only plans ------------------------------------------------------------------------------------
def _host_plan(*a, **kw):
    import recfilter_amd as rfa
    return rfa.Plan(*a, device=capi.RF_DEVICE_HOST_ONLY, **kw)


def test_debug_buffers_of_host_only_plans():
    """kinds and sizes without pointers; the buffers of child plans are listed behind the plan's own"""
    from recfilter_amd.capi import RecFilterError
    scans = rc.xy_pm(rc.GAUSS2)
    with _host_plan((128, 512), scans, clamped=True, path=fp.FUSED, flags=fp.TILED) as plan:
        bufs = plan.debug_buffers()
        assert [i for i, _, _ in bufs] == list(range(len(bufs)))
        kinds = [k for _, k, _ in bufs]
        assert set(kinds) == {"table", "zeroed", "scratch"}
        assert sum(b for _, _, b in bufs) == plan.workspace_bytes
        assert all(b > 0 for _, _, b in bufs)
        n32 = len(bufs)
        with pytest.raises(RecFilterError) as e:
            plan.debug_fill(kinds.index("table"), 0xFF)              # a table is never filled
        assert e.value.status == capi.RF_ERR_INVALID_ARG
        with pytest.raises(RecFilterError) as e:
            plan.debug_fill(kinds.index("scratch"), 0xFF)            # no device memory
        assert e.value.status == capi.RF_ERR_HIP
        for bad in (-1, len(bufs)):
            with pytest.raises(RecFilterError) as e:
                plan.debug_fill(bad, 0)
            assert e.value.status == capi.RF_ERR_INVALID_ARG
    # a staged 16-bit plan: its f32 planes (scratch) in front of the f32 plan's buffers
    with _host_plan((128, 516), scans, dtype=torch.float16, clamped=True, path=capi.RF_PATH_AUTO, flags=fp.TILED | capi.RF_PLAN_STAGE_HALF) as plan:
        bufs = plan.debug_buffers()
        assert bufs[0][1:] == ("scratch", 128 * 516 * 4)
        assert len(bufs) > 1 and "table" in [k for _, k, _ in bufs[1:]]
        assert sum(b for _, _, b in bufs) == plan.workspace_bytes
    # an in-plan cascade owns nothing itself: every buffer is a stage's
    with _host_plan((300, 1024), [(0, True, [0.5, 0.5])] * 5 + [(1, True, [0.5, 0.5])], flags=fp.TILED) as plan:
        bufs = plan.debug_buffers()
        assert len(bufs) > n32 and sum(b for _, _, b in bufs) == plan.workspace_bytes
    # a clamped 1-D signal: its own tables and dot products (zeroed), then the zero-border plan's
    with _host_plan((100_000,), [(0, True, rc.GAUSS2)], clamped=True, flags=fp.TILED) as plan:
        kinds = [k for _, k, _ in plan.debug_buffers()]
        assert kinds[:5] == ["table"] * 4 + ["zeroed"] and "scratch" in kinds[5:]
    # the one-read volume plan: the helper plan's buffers are listed
    with _host_plan((64, 96, 512), fp.XYZ, clamped=True, path=fp.FUSED, flags=capi.RF_PLAN_WALK_PASS1) as walk, \
            _host_plan((64, 96, 512), fp.XYZ, clamped=True, path=fp.FUSED, flags=capi.RF_PLAN_STAGED_PASS1) as two:
        assert len(walk.debug_buffers()) > len(two.debug_buffers())
        assert sum(b for _, _, b in walk.debug_buffers()) == walk.workspace_bytes


def test_every_footprint_row_reaches_its_instance():
    """path and tiles of every row of tests/test_gpu_footprint.py, as a host-only plan; the rows name every path and type"""
    wrong = []
    for name, r in fp.ROWS.items():
        with fp.make_plan(r, device=capi.RF_DEVICE_HOST_ONLY) as plan:
            try:
                fp.check_instance(r, plan)
            except AssertionError as e:
                wrong.append(str(e))
            assert int(np.prod(r["shape"])) <= fp.MAX_SAMPLES
    assert not wrong, wrong
    groups = {r["group"] for r in fp.ROWS.values()}
    for path in ("fused 2-D", "fused 3-D", "fused 1-D", "line-parallel untiled", "thread-per-line untiled", "generic tiled", "overlapped tiled",
                 "matrix", "staged", "uint8 input", "in-plan cascade", "fused sections"):
        assert any(g.startswith(path) for g in groups), path
    for kind in ("f32", "f64", "i32", "i16", "f16", "bf16"):
        assert any(g.endswith("/" + kind) for g in groups), kind
