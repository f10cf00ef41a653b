"""Byte planes on both sides (rf_input_dtype RF_IO_U8) on the host: the enum, the plan decisions of a host-only plan, the
refusals, and that the per-sample rule of tests/test_gpu_u8_output.py is one a correct f32 implementation passes.

RF_IO_U8 is a storage type: the plan is the RF_IN_U8 f32 plan of the same description and the result is converted once, so
everything a host-only plan shows of a native plan must be what that RF_IN_U8 plan shows; a staged plan shows one launch and
the f32 planes more."""
import ctypes

import numpy as np
import pytest

import ref_cases as rc
import recfilter_amd as rfa
import u8_cases as u8
from recfilter_amd import capi

HOST = dict(device=capi.RF_DEVICE_HOST_ONLY)
FUSED = capi.RF_PATH_TILED_FUSED
TILED = capi.RF_PLAN_TILED_ONLY
CFG3 = rc.xy_pm(rc.GAUSS2)
BYTES_IO = dict(dtype=np.float32, input_dtype=np.uint8, output_dtype=np.uint8)
BYTES_IN = dict(dtype=np.float32, input_dtype=np.uint8)


def _desc(dtype_code=capi.RF_F32, shape=(512, 1024), in_dtype=2, flags=TILED, shard_world=1):
    scans = CFG3
    arr = (capi.ScanDesc * len(scans))()
    for i, (dim, causal, coeff) in enumerate(scans):
        arr[i].dim, arr[i].causal, arr[i].order, arr[i].feedfwd = dim, int(causal), len(coeff) - 1, coeff[0]
        for j, c in enumerate(coeff[1:]):
            arr[i].feedback[j] = c
    d = capi.FilterDesc()
    d.abi, d.ndim, d.dtype, d.n_planes, d.n_scans = capi.RF_ABI, len(shape), dtype_code, 1, len(scans)
    for i, e in enumerate(reversed(shape)):
        d.extent[i] = e
    d.scans = ctypes.cast(arr, ctypes.POINTER(capi.ScanDesc))
    d.path, d.device = capi.RF_PATH_AUTO, capi.RF_DEVICE_HOST_ONLY
    d.border = capi.RF_BORDER_CLAMP
    d.shard_world = shard_world
    d.pointwise.in_dtype = in_dtype
    d.flags = flags
    return d, arr


def _create(d):
    h = ctypes.c_void_p()
    rc_ = capi.lib().rf_plan_create(ctypes.byref(d), ctypes.byref(h))
    if rc_ == capi.RF_OK:
        capi.lib().rf_plan_destroy(h)
    return rc_


def test_enum_value_abi_and_struct_size():
    assert capi.RF_IO_U8 == 2 and (capi.RF_IN_PIXEL, capi.RF_IN_U8) == (0, 1)
    d, keep = _desc(in_dtype=2)
    assert _create(d) == capi.RF_OK
    d, keep = _desc(in_dtype=3)
    assert _create(d) == capi.RF_ERR_INVALID_ARG
    assert b"abi 3" in capi.lib().rf_version() and capi.RF_ABI == 3
    assert ctypes.sizeof(capi.PointwiseDesc) == 28


def test_native_plan_is_the_u8_input_plan():
    kw = dict(clamped=True, flags=TILED, **HOST)
    with rfa.Plan((512, 1024), CFG3, **BYTES_IO, **kw) as p8, rfa.Plan((512, 1024), CFG3, **BYTES_IN, **kw) as pin:
        assert p8.path == FUSED and pin.path == FUSED
        assert p8.num_kernels == pin.num_kernels
        assert p8.tiles == pin.tiles
        assert p8.workspace_bytes == pin.workspace_bytes
        for t in ("H_x", "H_y", "W_x", "A_y", "G_x", "scans", "neighbour_carries"):
            assert np.array_equal(p8.table(t), pin.table(t)), t


@pytest.mark.parametrize("shape,scans,clamped,flags", [
    ((64, 250), CFG3, True, TILED),
    ((40, 16, 272), rc.REFERENCE_TESTS["test_generic_xyz"]["scans"], False, TILED),
    ((512, 1024), CFG3, True, TILED | capi.RF_PLAN_STAGE_HALF),
], ids=["odd_width", "volume", "stage_half_flag"])
def test_staged_plans_add_one_launch_and_the_f32_planes(shape, scans, clamped, flags):
    kw = dict(clamped=clamped, flags=flags, **HOST)
    with rfa.Plan(shape, scans, **BYTES_IO, **kw) as p8, rfa.Plan(shape, scans, **BYTES_IN, **kw) as pin:
        assert p8.num_kernels == pin.num_kernels + 1
        assert p8.workspace_bytes >= int(np.prod(shape)) * 4
        assert p8.workspace_bytes == pin.workspace_bytes + int(np.prod(shape)) * 4
        assert p8.path == pin.path
        kinds = [k for _, k, _ in p8.debug_buffers()]
        assert "scratch" in kinds           # the staging planes


def test_stage_half_changes_nothing_for_a_plan_without_byte_output():
    for extra in (BYTES_IN, dict(dtype=np.float32)):
        with rfa.Plan((512, 1024), CFG3, clamped=True, flags=TILED | capi.RF_PLAN_STAGE_HALF, **extra, **HOST) as a, \
             rfa.Plan((512, 1024), CFG3, clamped=True, flags=TILED, **extra, **HOST) as b:
            assert a.num_kernels == b.num_kernels and a.workspace_bytes == b.workspace_bytes and a.path == b.path


@pytest.mark.parametrize("code", [capi.RF_F64, capi.RF_F16, capi.RF_BF16], ids=["f64", "f16", "bf16"])
def test_other_pixel_types_are_unsupported(code):
    d, keep = _desc(dtype_code=code)
    assert _create(d) == capi.RF_ERR_UNSUPPORTED


def test_sharded_plans_are_unsupported():
    d, keep = _desc(shard_world=2)
    assert _create(d) == capi.RF_ERR_UNSUPPORTED
    d, keep = _desc(flags=TILED | capi.RF_PLAN_FORCE_EXCHANGE)
    assert _create(d) == capi.RF_ERR_UNSUPPORTED


def test_python_types():
    import torch
    for dt in (np.uint8, torch.uint8):
        with rfa.Plan((256, 512), CFG3, dtype=np.float32, input_dtype=dt, output_dtype=dt, **HOST) as p:
            assert p.output_np_dtype == np.dtype(np.uint8) and p.input_np_dtype == np.dtype(np.uint8)
    with pytest.raises(TypeError):
        rfa.Plan((256, 512), CFG3, dtype=np.float32, output_dtype=np.uint8, **HOST)                       # no byte input
    with pytest.raises(TypeError):
        rfa.Plan((256, 512), CFG3, dtype=np.float64, input_dtype=np.uint8, output_dtype=np.uint8, **HOST)  # not float32
    with pytest.raises(TypeError):
        rfa.Plan((256, 512), CFG3, dtype=np.float32, input_dtype=np.uint8, output_dtype=np.float32, **HOST)


def test_to_bytes_consumer_needs_a_byte_definition():
    import torch
    from recfilter_amd.filter import RecFilter, RecFilterDim, Pointwise, RecFilterUsageError
    x, y = RecFilterDim("x", 64), RecFilterDim("y", 32)
    f = RecFilter("F")
    f.define([x, y], torch.zeros((32, 64), dtype=torch.float32))
    with pytest.raises(RecFilterUsageError):
        f.compute_at(Pointwise(255.0, to_bytes=True))


# ---- the rule of the GPU test is one a correct f32 implementation passes --------------------------------------------------
@pytest.mark.parametrize("case", u8.GAUSS_CASES, ids=u8.GAUSS_IDS)
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
@pytest.mark.parametrize("setup", u8.SETUPS, ids=u8.SETUP_IDS)
def test_the_f32_oracle_passes_the_one_rounding_rule(case, clamped, setup):
    """sat8 of the oracle run in f32 on the GPU test's inputs and seeds obeys |got - clip(want)| <= 0.5 + 1e-4 * scale"""
    (shape, _, _), coeff = u8.NATIVE_SHAPES[case[0]], getattr(rc, case[1])
    _, prologue, epilogue = setup
    scans = rc.xy_pm(coeff)
    for plane in range(3):
        img = u8.byte_image(shape, u8.seed_of(shape, plane))
        want, scale = u8.want_and_scale(img, scans, clamped, prologue, epilogue)
        got = u8.f32_reference_bytes(img, scans, clamped, prologue, epilogue)
        excess = u8.rule_excess(got, want, scale)
        assert excess <= 0.0, f"plane {plane}: the f32 oracle misses the rule by {excess}"


@pytest.mark.parametrize("shape,scans,name", u8.STAGED_SHAPES, ids=[s[2] for s in u8.STAGED_SHAPES])
def test_the_f32_oracle_passes_the_rule_on_the_staged_shapes(shape, scans, name):
    clamped = name == "odd_width"
    img = u8.byte_image(shape, u8.seed_of(shape))
    want, scale = u8.want_and_scale(img, scans, clamped)
    assert u8.rule_excess(u8.f32_reference_bytes(img, scans, clamped), want, scale) <= 0.0


def test_sat8_reference():
    v = np.array([-3.0, -0.5, 0.5, 1.5, 2.5, 254.5, 255.5, 1e9, np.nan], dtype=np.float32)
    assert u8.sat8(v).tolist() == [0, 0, 0, 2, 2, 254, 255, 255, 0]
