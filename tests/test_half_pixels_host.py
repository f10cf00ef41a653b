"""16-bit float pixels (RF_F16, RF_BF16) on the host: the enum, the plan decisions of a host-only plan and the refusals.
The two types are STORAGE types -- out = round16(F_f32(widen(in))) -- so everything a host-only plan shows of such a plan
(path, tiles, tables, the neighbour-carry decision) must be what the f32 plan of the same description shows."""
import ctypes

import numpy as np
import pytest

import ref_cases as rc
import recfilter_amd as rfa
from recfilter_amd import capi

HOST = dict(device=capi.RF_DEVICE_HOST_ONLY)
FUSED = capi.RF_PATH_TILED_FUSED
TILED = capi.RF_PLAN_TILED_ONLY


def _dtypes():
    import torch
    return [("f16", torch.float16, capi.RF_F16), ("bf16", torch.bfloat16, capi.RF_BF16)]


DTYPES = _dtypes()
IDS = [d[0] for d in DTYPES]


def _desc(dtype_code, shape=(512, 1024), in_dtype=capi.RF_IN_PIXEL):
    scans = rc.xy_pm(rc.GAUSS2)
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
    d.pointwise.in_dtype = in_dtype
    d.flags = TILED
    return d, arr


def test_enum_values_and_abi():
    assert (capi.RF_F32, capi.RF_F64, capi.RF_I32, capi.RF_I16, capi.RF_F16, capi.RF_BF16) == (0, 1, 2, 3, 4, 5)
    assert b"abi 3" in capi.lib().rf_version()


def test_dtype_6_is_an_invalid_argument():
    d, keep = _desc(6)
    h = ctypes.c_void_p()
    assert capi.lib().rf_plan_create(ctypes.byref(d), ctypes.byref(h)) == capi.RF_ERR_INVALID_ARG


@pytest.mark.parametrize("name,tdt,code", DTYPES, ids=IDS)
def test_u8_input_is_unsupported(name, tdt, code):
    d, keep = _desc(code, in_dtype=capi.RF_IN_U8)
    h = ctypes.c_void_p()
    assert capi.lib().rf_plan_create(ctypes.byref(d), ctypes.byref(h)) == capi.RF_ERR_UNSUPPORTED


@pytest.mark.parametrize("name,tdt,code", DTYPES, ids=IDS)
@pytest.mark.parametrize("coeff", ["GAUSS2", "GAUSS3", "BICUBIC_COEFF"])
@pytest.mark.parametrize("clamped", [True, False], ids=["clamped", "zero"])
@pytest.mark.parametrize("shape,rows", [((4 * 128, 8 * 256), 128), ((2 * 128 + 70, 5 * 256), 128), ((512, 1028), 64), ((96, 512), 32),
                                        ((16384, 16384), 0)],
                         ids=["whole128", "partial128", "rows64", "rows32", "cfg3_size"])
def test_fused_plan_is_the_f32_plan(name, tdt, code, coeff, clamped, shape, rows):
    scans = rc.xy_pm(getattr(rc, coeff))
    flags = TILED | (capi.RF_PLAN_TILE_ROWS(rows) if rows else 0)
    with rfa.Plan(shape, scans, dtype=tdt, clamped=clamped, path=FUSED, flags=flags, **HOST) as p16, \
         rfa.Plan(shape, scans, dtype=np.float32, clamped=clamped, path=FUSED, flags=flags, **HOST) as p32:
        assert p16.path == FUSED and p32.path == FUSED
        assert p16.tiles == p32.tiles
        assert np.array_equal(p16.table("neighbour_carries"), p32.table("neighbour_carries"))
        # cast_coeff does not round the coefficients to 16 bits
        assert np.array_equal(p16.table("scans"), p32.table("scans"))
        assert p16.num_kernels == p32.num_kernels
        for t in ("H_x", "H_y", "W_x", "A_y", "G_x"):
            assert np.array_equal(p16.table(t), p32.table(t))


@pytest.mark.parametrize("name,tdt,code", DTYPES, ids=IDS)
def test_auto_path_of_a_small_image_stays_on_one_rounding(name, tdt, code):
    """The automatic path sends a small f32 image to the line kernels (x stage, then y stage through the output planes); a
    16-bit plan must not do that natively."""
    scans = rc.xy_pm(rc.GAUSS2)
    with rfa.Plan((512, 512), scans, dtype=tdt, flags=0, **HOST) as p16, rfa.Plan((512, 512), scans, dtype=np.float32, flags=0, **HOST) as p32:
        assert p32.path == capi.RF_PATH_UNTILED
        assert p16.path == FUSED


@pytest.mark.parametrize("name,tdt,code", DTYPES, ids=IDS)
def test_z_sharded_volume_is_unsupported(name, tdt, code):
    scans = rc.xy_pm(rc.GAUSS2) + [(2, True, rc.GAUSS2)]
    with pytest.raises(capi.RecFilterError) as e:
        rfa.Plan((64, 96, 128), scans, dtype=tdt, shard_rank=0, shard_world=2, **HOST)
    assert e.value.status == capi.RF_ERR_UNSUPPORTED


@pytest.mark.parametrize("name,tdt,code", DTYPES, ids=IDS)
def test_row_sharded_image_is_native(name, tdt, code):
    with rfa.Plan((256, 512), rc.xy_pm(rc.GAUSS2), dtype=tdt, clamped=True, path=FUSED, shard_rank=1, shard_world=2, **HOST) as p:
        assert p.path == FUSED and p.num_exchanges >= 1


@pytest.mark.parametrize("name,tdt,code", DTYPES, ids=IDS)
def test_plans_outside_the_native_path_are_created(name, tdt, code):
    g2 = rc.xy_pm(rc.GAUSS2)
    order5 = [1.0 - 0.5, 0.1, 0.1, 0.1, 0.1, 0.1]
    cases = [((64, 96, 128), g2 + [(2, True, rc.GAUSS2), (2, False, rc.GAUSS2)], False),
             ((256, 512), [(0, True, order5), (0, False, order5), (1, True, order5), (1, False, order5)], True),
             ((300, 1001), g2, True)]
    for shape, scans, clamped in cases:
        with rfa.Plan(shape, scans, dtype=tdt, clamped=clamped, **HOST) as p:
            assert p.num_kernels >= 3
            assert p.workspace_bytes >= int(np.prod(shape)) * 4        # the f32 planes of a staged plan


def test_python_dtypes_construct():
    import torch
    for dt, code in ((np.float16, capi.RF_F16), (torch.float16, capi.RF_F16), (torch.bfloat16, capi.RF_BF16)):
        with rfa.Plan((256, 512), rc.xy_pm(rc.GAUSS2), dtype=dt, **HOST) as p:
            assert p.dtype_code == code
    with rfa.Plan((256, 512), rc.xy_pm(rc.GAUSS2), dtype=torch.bfloat16, **HOST) as p:
        assert p.np_dtype is None           # numpy has no bfloat16
    with rfa.Plan((256, 512), rc.xy_pm(rc.GAUSS2), dtype=np.float16, **HOST) as p:
        assert p.np_dtype == np.dtype(np.float16)


def test_stage_half_flag_is_ignored_for_f32_and_stages_a_16_bit_plan():
    import torch
    g2 = rc.xy_pm(rc.GAUSS2)
    with rfa.Plan((512, 1024), g2, dtype=np.float32, path=FUSED, flags=TILED | capi.RF_PLAN_STAGE_HALF, **HOST) as a, \
         rfa.Plan((512, 1024), g2, dtype=np.float32, path=FUSED, flags=TILED, **HOST) as b:
        assert a.num_kernels == b.num_kernels and a.workspace_bytes == b.workspace_bytes
    with rfa.Plan((512, 1024), g2, dtype=torch.float16, flags=TILED | capi.RF_PLAN_STAGE_HALF, **HOST) as a, \
         rfa.Plan((512, 1024), g2, dtype=torch.float16, flags=TILED, **HOST) as b:
        assert a.num_kernels == b.num_kernels + 2 and a.workspace_bytes >= b.workspace_bytes + 512 * 1024 * 4
