"""CPU tests of the batched smoothing plan (rf_smooth_plan_create_batched, recfilter_amd.SmoothPlan(batch=N)): the symbol, the
refusals at create in the order the header documents (decided before any HIP call), launch counts that do not depend on the
batch, workspaces that are exactly `batch` times the single-image plan's, and what a host-only plan answers.  No kernel is
launched."""
import ctypes
import os

import pytest

import recfilter_amd as rfa
import smooth_cases as sc
from recfilter_amd import capi

HOST = capi.RF_DEVICE_HOST_ONLY
INVALID, UNSUPPORTED, HIP = capi.RF_ERR_INVALID_ARG, capi.RF_ERR_UNSUPPORTED, capi.RF_ERR_HIP
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "recfilter_amd.h")


def desc(**over):
    d = capi.SmoothDesc()
    d.abi, d.image_u8, d.width, d.height, d.n_planes, d.n_guide, d.guide_u8 = capi.RF_ABI, 0, 64, 40, 1, 0, 0
    d.iterations, d.sigma_s, d.sigma_r, d.device, d.flags = 3, 40.0, 0.5, HOST, 0
    for k, v in over.items():
        setattr(d, k, v)
    return d


def batch_desc(d, batch, image_stride=None, guide_stride=None):
    b = capi.SmoothBatchDesc()
    b.batch = batch
    b.image_stride = d.n_planes * d.width * d.height if image_stride is None else image_stride
    b.guide_stride = d.n_guide * d.width * d.height if guide_stride is None else guide_stride
    return b


def create(d, b):
    """(status, handle, message) of rf_smooth_plan_create_batched; b=None passes a null batch"""
    h = ctypes.c_void_p(0xdead)      # (the call must clear it)
    rc = capi.lib().rf_smooth_plan_create_batched(ctypes.byref(d), ctypes.byref(b) if b is not None else None, ctypes.byref(h))
    return rc, h, capi.lib().rf_last_error_string().decode()


def single(d):
    h = ctypes.c_void_p()
    capi.check(capi.lib().rf_smooth_plan_create(ctypes.byref(d), ctypes.byref(h)))
    return h


# ---- the symbol -----------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_typed():
    name = "rf_smooth_plan_create_batched"
    assert name in capi.EXPORTED_SYMBOLS
    fn = getattr(capi.lib(), name)                               # resolves in the built library, or raises
    assert fn.argtypes is not None and len(fn.argtypes) == 3
    header = open(HEADER).read()
    assert f" {name}(" in header and "rf_smooth_batch_desc" in header
    assert "#define RF_SMOOTH_MAX_BATCH 1024" in header and capi.RF_SMOOTH_MAX_BATCH == 1024
    assert [f[0] for f in capi.SmoothBatchDesc._fields_] == ["batch", "image_stride", "guide_stride"]
    assert capi.RF_ABI == 3                                      # (the batch came without a new revision)


# ---- refusals at create -----------------------------------------------------------------------------------------------------------
S = 64 * 40
BATCH_REFUSALS = [
    ("batch 0", dict(), dict(batch=0), INVALID, "batch must be 1..1024"),
    ("batch -1", dict(), dict(batch=-1), INVALID, "batch must be 1..1024"),
    ("batch 1025", dict(), dict(batch=capi.RF_SMOOTH_MAX_BATCH + 1), INVALID, "batch must be 1..1024"),
    ("image stride not a multiple of 4", dict(), dict(batch=2, image_stride=S + 2), INVALID, "multiples of 4"),
    ("guide stride not a multiple of 4", dict(n_guide=1), dict(batch=2, guide_stride=S + 1), INVALID, "multiples of 4"),
    ("image stride below a plane", dict(), dict(batch=2, image_stride=S - 4), INVALID, "image_stride"),
    ("image stride 0", dict(), dict(batch=2, image_stride=0), INVALID, "image_stride"),
    ("guide stride without a guide", dict(), dict(batch=2, guide_stride=S), INVALID, "guide_stride must be 0"),
    ("guide stride below a plane", dict(n_guide=1), dict(batch=2, guide_stride=S - 4), INVALID, "guide_stride"),
    ("a guide shared by the batch", dict(n_guide=1), dict(batch=2, guide_stride=0), INVALID, "shared"),
    # the plain create's refusals, reached through the batched call
    ("width 66", dict(width=66), dict(batch=2, image_stride=66 * 40), UNSUPPORTED, "multiple of 4"),
    ("flags", dict(flags=1), dict(batch=2), INVALID, "flags"),
    ("n_planes 17", dict(n_planes=capi.RF_MAX_PLANES + 1), dict(batch=2), INVALID, "n_planes"),
]


@pytest.mark.parametrize("what,over,batch,status,text", BATCH_REFUSALS, ids=[r[0] for r in BATCH_REFUSALS])
def test_create_refusals(what, over, batch, status, text):
    d = desc(**over)
    rc, h, message = create(d, batch_desc(d, **batch))
    assert rc == status, (what, rc, message)
    assert text in message, (what, message)
    assert not h.value, "a refused create left a handle"


def test_null_batch_is_refused():
    rc, h, message = create(desc(), None)
    assert rc == INVALID and "batch" in message and not h.value


def test_refusals_come_in_the_documented_order():
    """a description that breaks several rules answers with the first of them"""
    d = desc(flags=1, width=66)
    for b, text in ((dict(batch=0, image_stride=2), "batch must be"), (dict(batch=2, image_stride=2), "multiples of 4"),
                    (dict(batch=2, image_stride=4), "image_stride"), (dict(batch=2, image_stride=66 * 40, guide_stride=4), "guide_stride must be 0"),
                    (dict(batch=2, image_stride=66 * 40), "flags")):
        rc, h, message = create(d, batch_desc(d, **b))
        assert rc == INVALID and text in message and not h.value, (b, message)


# ---- launch counts and workspaces -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 2, 7])
@pytest.mark.parametrize("K", [1, 3])
def test_launch_counts_do_not_grow_with_the_batch(batch, K):
    L = capi.lib()
    d = desc(iterations=K, n_planes=3, n_guide=2)
    one = single(d)
    rc, h, message = create(d, batch_desc(d, batch))
    assert rc == capi.RF_OK, message
    try:
        assert L.rf_smooth_plan_num_kernels(h) == L.rf_smooth_plan_num_kernels(one) == 1 + 6 * K
        assert L.rf_smooth_plan_backward_num_kernels(h, 0) == L.rf_smooth_plan_backward_num_kernels(one, 0) == 1 + 12 * K
        assert L.rf_smooth_plan_backward_num_kernels(h, 1) == L.rf_smooth_plan_backward_num_kernels(one, 1) == 34 * K - 4
        a, b = (ctypes.c_float * K)(), (ctypes.c_float * K)()
        capi.check(L.rf_smooth_plan_bases(h, a))
        capi.check(L.rf_smooth_plan_bases(one, b))
        assert list(a) == list(b)
    finally:
        L.rf_smooth_plan_destroy(h)
        L.rf_smooth_plan_destroy(one)


@pytest.mark.parametrize("u8", [0, 1], ids=["f32", "uint8"])
@pytest.mark.parametrize("shape", sc.SHAPES, ids=[str(s) for s in sc.SHAPES])
def test_workspaces_are_batch_times_the_single_plans(shape, u8):
    L = capi.lib()
    C, H, W = shape
    d = desc(n_planes=C, height=H, width=W, image_u8=u8)
    one = single(d)
    try:
        w1, b0, b1 = L.rf_smooth_plan_workspace_bytes(one), L.rf_smooth_plan_backward_workspace_bytes(one, 0), L.rf_smooth_plan_backward_workspace_bytes(one, 1)
        assert w1 > 0 and b0 == 0 and b1 > 0
        for batch in (1, 2, 7):
            rc, h, message = create(d, batch_desc(d, batch, image_stride=C * H * W + 8))
            assert rc == capi.RF_OK, message
            try:
                assert L.rf_smooth_plan_workspace_bytes(h) == batch * w1
                assert L.rf_smooth_plan_backward_workspace_bytes(h, 0) == 0
                assert L.rf_smooth_plan_backward_workspace_bytes(h, 1) == batch * b1
            finally:
                L.rf_smooth_plan_destroy(h)
    finally:
        L.rf_smooth_plan_destroy(one)


# ---- a host-only plan ---------------------------------------------------------------------------------------------------------------
def test_host_only_batched_plan_refuses_to_run_after_the_array_checks():
    L = capi.lib()
    d = desc(n_planes=2, n_guide=1)
    rc, h, message = create(d, batch_desc(d, 3))
    assert rc == capi.RF_OK, message
    two, one = (ctypes.c_void_p * 2)(), (ctypes.c_void_p * 1)()
    try:
        assert L.rf_smooth_plan_execute(h, two, None, two, None) == INVALID          # the guide array first
        assert "guide_planes is null" in L.rf_last_error_string().decode()
        assert L.rf_smooth_plan_execute(h, two, one, two, None) == HIP
        assert "host-only" in L.rf_last_error_string().decode()
        assert L.rf_smooth_plan_backward(h, two, one, two, two, one, 0, None) == INVALID      # edges = 0 takes no guide gradient
        assert L.rf_smooth_plan_backward(h, two, one, two, two, None, 0, None) == HIP
        assert "host-only" in L.rf_last_error_string().decode()
        assert L.rf_smooth_plan_backward(h, two, one, two, two, one, 1, None) == HIP
    finally:
        L.rf_smooth_plan_destroy(h)


# ---- Python -------------------------------------------------------------------------------------------------------------------------
def test_python_plan_reports_the_library_text():
    with pytest.raises(capi.RecFilterError, match=r"batch must be 1\.\.1024 \(got 0\)") as e:
        rfa.SmoothPlan((40, 64), device=HOST, batch=0)
    assert e.value.status == INVALID


def test_python_plan_queries():
    with rfa.SmoothPlan((40, 64), planes=3, iterations=2, device=HOST) as one, rfa.SmoothPlan((40, 64), planes=3, iterations=2, device=HOST, batch=5) as plan:
        assert plan.batch == 5 and one.batch is None
        assert plan.num_kernels == one.num_kernels == 13
        assert plan.backward_num_kernels(True) == one.backward_num_kernels(True) == 64
        assert plan.workspace_bytes == 5 * one.workspace_bytes
        assert plan.backward_workspace_bytes(True) == 5 * one.backward_workspace_bytes(True)
        assert plan.bases == one.bases
        with pytest.raises(capi.RecFilterError, match="host-only"):
            plan.execute(None)
