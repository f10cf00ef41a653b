"""CPU tests of the smoothing plan (rf_smooth_plan_*, recfilter_amd.SmoothPlan): the symbols, the refusals at create (decided
before any HIP call), what a host-only plan answers, and the self-check of the byte rule of tests/smooth_cases.py -- the f32
serial loop's sat8 satisfies it, a filter that rounds to bytes between iterations violates it.  No kernel is launched."""
import ctypes

import numpy as np
import pytest

import recfilter_amd as rfa
import smooth_cases as sc
from recfilter_amd import capi

HOST = capi.RF_DEVICE_HOST_ONLY

# ---- symbols ----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["rf_smooth_plan_create", "rf_smooth_plan_destroy", "rf_smooth_plan_workspace_bytes", "rf_smooth_plan_num_kernels",
               "rf_smooth_plan_bases", "rf_smooth_plan_execute", "rf_smooth_plan_execute_timed"]


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_symbols_are_exported_declared_and_typed(name):
    assert name in capi.EXPORTED_SYMBOLS
    fn = getattr(capi.lib(), name)                               # resolves in the built library, or raises
    assert fn.argtypes is not None, f"{name} has no argtypes in capi.py"
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "recfilter_amd.h")).read()
    assert f" {name}(" in header


def test_python_names_are_exported():
    assert "SmoothPlan" in rfa.__all__ and hasattr(rfa, "SmoothPlan")
    for name in ("execute", "execute_timed", "bases", "workspace_bytes", "num_kernels", "close", "__enter__", "__exit__"):
        assert hasattr(rfa.SmoothPlan, name), name
    assert capi.RF_ABI == 3 and capi.RF_SMOOTH_MAX_ITERATIONS == 8
    assert capi.lib().rf_smooth_plan_workspace_bytes.restype is ctypes.c_size_t


# ---- refusals at create -----------------------------------------------------------------------------------------------------
def desc(**over):
    d = capi.SmoothDesc()
    d.abi, d.image_u8, d.width, d.height, d.n_planes, d.n_guide, d.guide_u8 = capi.RF_ABI, 0, 64, 40, 1, 0, 0
    d.iterations, d.sigma_s, d.sigma_r, d.device, d.flags = 3, 40.0, 0.5, HOST, 0
    for k, v in over.items():
        setattr(d, k, v)
    return d


INVALID, UNSUPPORTED = capi.RF_ERR_INVALID_ARG, capi.RF_ERR_UNSUPPORTED
CREATE_REFUSALS = [
    ("abi", dict(abi=capi.RF_ABI + 1), INVALID), ("flags", dict(flags=1), INVALID),
    ("n_planes 0", dict(n_planes=0), INVALID), ("n_planes 17", dict(n_planes=capi.RF_MAX_PLANES + 1), INVALID),
    ("n_guide -1", dict(n_guide=-1), INVALID), ("n_guide 17", dict(n_guide=capi.RF_MAX_PLANES + 1), INVALID),
    ("image_u8 2", dict(image_u8=2), INVALID), ("image_u8 -1", dict(image_u8=-1), INVALID),
    ("guide_u8 2", dict(n_guide=1, guide_u8=2), INVALID), ("guide_u8 without a guide", dict(n_guide=0, guide_u8=1), INVALID),
    ("iterations 0", dict(iterations=0), INVALID), ("iterations 9", dict(iterations=capi.RF_SMOOTH_MAX_ITERATIONS + 1), INVALID),
    ("width 0", dict(width=0), INVALID), ("height 0", dict(height=0), INVALID), ("height -3", dict(height=-3), INVALID),
    ("sigma_s 0", dict(sigma_s=0.0), INVALID), ("sigma_s negative", dict(sigma_s=-1.0), INVALID),
    ("sigma_s NaN", dict(sigma_s=float("nan")), INVALID), ("sigma_s infinite", dict(sigma_s=float("inf")), INVALID),
    ("sigma_r 0", dict(sigma_r=0.0), INVALID), ("sigma_r NaN", dict(sigma_r=float("nan")), INVALID),
    ("sigma_r infinite", dict(sigma_r=float("inf")), INVALID),
    ("width 66", dict(width=66), UNSUPPORTED), ("width above 2^21", dict(width=(1 << 21) + 4, height=1), UNSUPPORTED),
    ("height above 2^21", dict(width=4, height=(1 << 21) + 1), UNSUPPORTED),
    ("a_k rounds to 1", dict(sigma_s=1e9), UNSUPPORTED), ("a_k rounds to 0", dict(sigma_s=1e-3), UNSUPPORTED),
]


@pytest.mark.parametrize("what,over,want", CREATE_REFUSALS, ids=[c[0] for c in CREATE_REFUSALS])
def test_create_refusals(what, over, want):
    lib = capi.lib()
    handle = ctypes.c_void_p(0xdead)
    d = desc(**over)
    status = lib.rf_smooth_plan_create(ctypes.byref(d), ctypes.byref(handle))
    message = lib.rf_last_error_string().decode()
    assert status == want, f"{what}: status {status} ({message})"
    assert message, f"{what}: no text in rf_last_error_string"
    assert not handle.value, f"{what}: a refused create left a handle"
    if what.startswith("a_k"):
        assert "k = " in message, message


def test_create_refuses_null_arguments():
    lib = capi.lib()
    handle = ctypes.c_void_p()
    d = desc()
    assert lib.rf_smooth_plan_create(None, ctypes.byref(handle)) == INVALID
    assert lib.rf_smooth_plan_create(ctypes.byref(d), None) == INVALID
    assert lib.rf_smooth_plan_destroy(None) == capi.RF_OK
    assert lib.rf_smooth_plan_num_kernels(None) == 0 and lib.rf_smooth_plan_workspace_bytes(None) == 0
    assert lib.rf_smooth_plan_bases(None, None) == INVALID


def test_python_constructor_raises_the_library_text():
    with pytest.raises(rfa.RecFilterError) as e:
        rfa.SmoothPlan((40, 66), device=HOST)
    assert e.value.status == UNSUPPORTED and "multiple of 4" in str(e.value)
    import torch
    with pytest.raises(TypeError):
        rfa.SmoothPlan((40, 64), image_dtype=torch.float16, device=HOST)


# ---- host-only plans --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 8])
def test_num_kernels(K):
    with rfa.SmoothPlan((40, 64), iterations=K, device=HOST) as plan:
        assert plan.num_kernels == 1 + 6 * K


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("shape", sc.SHAPES, ids=str)
def test_workspace_is_the_sum_of_its_parts(shape, u8):
    import torch
    C, H, W = shape
    with rfa.SmoothPlan((H, W), planes=C, image_dtype=torch.uint8 if u8 else torch.float32, device=HOST) as plan, \
            rfa.VarPlan((H, W), sc.SCANS, planes=C, n_weights=2, device=HOST) as inner:
        assert plan.workspace_bytes == 8 * W * H + (4 * W * H * C if u8 else 0) + inner.workspace_bytes


@pytest.mark.parametrize("sigma_s,K", [(40.0, 3), (60.0, 1), (7.5, 5), (60.0, 8)])
def test_bases(sigma_s, K):
    with rfa.SmoothPlan((40, 64), iterations=K, sigma_s=sigma_s, device=HOST) as plan:
        got = np.array(plan.bases, dtype=np.float32)
    want = np.array(sc.bases_f32(sigma_s, K), dtype=np.float32)
    assert len(got) == K
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want).astype(np.float64)), (got, want)
    assert np.all(got[1:] < got[:-1]) and np.all((got > 0) & (got < 1))


@pytest.mark.parametrize("guide_planes", [0, 2])
def test_host_only_plan_refuses_to_execute(guide_planes):
    import torch
    with rfa.SmoothPlan((40, 64), guide_planes=guide_planes, guide_dtype=torch.uint8, image_dtype=torch.uint8, device=HOST) as plan:
        for call in (plan.execute, plan.execute_timed):
            with pytest.raises(rfa.RecFilterError) as e:
                call(None)
            assert e.value.status == capi.RF_ERR_HIP, str(e.value)
        # the checks of the arrays come first
        nulls = (ctypes.c_void_p * 2)()
        lib = capi.lib()
        assert lib.rf_smooth_plan_execute(plan._h, None, nulls if guide_planes else None, nulls, None) == INVALID
        assert lib.rf_smooth_plan_execute(plan._h, nulls, None if guide_planes else nulls, nulls, None) == INVALID
        assert lib.rf_smooth_plan_execute(None, nulls, None, nulls, None) == INVALID
        assert lib.rf_smooth_plan_execute_timed(plan._h, nulls, nulls if guide_planes else None, nulls, None, None, None, 0) == INVALID


# ---- the byte rule can fail -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.SHAPES[:3], ids=str)
def test_byte_rule_passes_the_serial_loop_and_catches_rounding_between_iterations(shape):
    K = 3
    img = sc.byte_image(shape)
    ds = sc.distances_f32(img, sc.SIGMA_S / sc.SIGMA_R / 255.0)
    bases = sc.bases_f32(sc.SIGMA_S, K)
    want, serial, abs_err32 = sc.truth_and_yardstick(img, ds, bases)
    margin = 255.0 * max(4 * abs_err32 / 255.0, 1e-6)
    once = sc.byte_rule_excess(sc.sat8(serial), want, abs_err32, f"{shape}: sat8 of the f32 serial loop")
    # the one rounding costs at most 0.5 + the serial loop's own error: three quarters of the f32 margin are left
    assert once <= -0.75 * margin + 1e-12, once
    between = sc.byte_rule_excess(sc.sat8(sc.filter_loops(img, ds, bases, np.float32, round_between=True)), want, abs_err32,
                                  f"{shape}: rounded to bytes between the iterations")
    assert between > 0, f"the rule does not see a filter that rounds between iterations (excess {between})"
