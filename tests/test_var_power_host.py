"""CPU tests of the power form of the spatially varying scans and of rf_var_distances: the argument checks that are decided
before any HIP call (host-only plans, host pointers), the bases of the domain-transform filter, the conversion
w = exp2(d * log2(base)) at its two exact points, and the exported symbols.  No kernel is launched."""
import ctypes
import math

import numpy as np
import pytest

import recfilter_amd as rfa
from recfilter_amd import capi

BASES = [0.5, 0.9, 0.98]
SCANS = [(0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1)]


def host_plan(n_weights=2):
    return rfa.VarPlan((64, 64), SCANS if n_weights == 2 else SCANS[:2], n_weights=n_weights, device=capi.RF_DEVICE_HOST_ONLY)


# ---- rf_var_plan_execute_power on a host-only plan --------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0.0, 1.0, 1.5, float("nan"), -0.5, float("inf")])
@pytest.mark.parametrize("where", [0, 1])
def test_bad_base_is_refused_and_named(bad, where):
    bases = [0.5, 0.5]
    bases[where] = bad
    with host_plan() as plan:
        for call in (plan.execute_power, plan.execute_power_timed):
            with pytest.raises(rfa.RecFilterError) as e:
                call([], [], bases)
            assert e.value.status == capi.RF_ERR_INVALID_ARG, str(e.value)
            assert f"plane {where}" in str(e.value)


def test_good_bases_reach_the_host_only_refusal():
    with host_plan() as plan:
        for call in (plan.execute_power, plan.execute_power_timed):
            with pytest.raises(rfa.RecFilterError) as e:
                call([], [], [0.5, 0.98])
            assert e.value.status == capi.RF_ERR_HIP
        with pytest.raises(ValueError):
            plan.execute_power([], [], [0.5])                    # one base per exponent plane


def test_null_arrays_come_first():
    lib = capi.lib()
    with host_plan(1) as plan:
        nulls = (ctypes.c_void_p * 1)()
        bad = (ctypes.c_float * 1)(2.0)
        assert lib.rf_var_plan_execute_power(plan._h, nulls, nulls, None, nulls, None) == capi.RF_ERR_INVALID_ARG
        assert lib.rf_var_plan_execute_power(plan._h, None, nulls, bad, nulls, None) == capi.RF_ERR_INVALID_ARG
        assert "null" in lib.rf_last_error_string().decode()
        assert lib.rf_var_plan_execute_power(None, nulls, nulls, bad, nulls, None) == capi.RF_ERR_INVALID_ARG
        assert plan.num_kernels == 3                              # the plan answers its queries as before


# ---- rf_var_distances: refusals, all before any HIP call --------------------------------------------------------------------
def aligned(nbytes, offset=0):
    """(keep-alive buffer, address): host memory on a 64-byte boundary, plus `offset`"""
    buf = np.zeros(nbytes + 128, dtype=np.uint8)
    at = (-buf.ctypes.data) % 64
    return buf, buf.ctypes.data + at + offset


def distances(guides, n_guide, u8, width, height, scale, dx, dy):
    arr = (ctypes.c_void_p * max(len(guides), 1))(*guides) if guides is not None else None
    status = capi.lib().rf_var_distances(arr, n_guide, u8, width, height, scale, dx, dy, -1, None)
    return status, capi.lib().rf_last_error_string().decode()


W, H = 16, 8
PLANE = W * H * 4


def test_distances_refusals():
    keep = [aligned(PLANE) for _ in range(3)]
    g, dx, dy = (a for _, a in keep)
    many = [g] * (capi.RF_MAX_PLANES + 1)
    cases = [
        ("width 6", ([g], 1, 0, 6, H, 1.0, dx, dy), capi.RF_ERR_UNSUPPORTED),
        ("width above the limit", ([g], 1, 0, (1 << 21) + 4, 1, 1.0, dx, dy), capi.RF_ERR_UNSUPPORTED),
        ("height above the limit", ([g], 1, 0, 4, (1 << 21) + 1, 1.0, dx, dy), capi.RF_ERR_UNSUPPORTED),
        ("n_guide 0", ([g], 0, 0, W, H, 1.0, dx, dy), capi.RF_ERR_INVALID_ARG),
        ("n_guide 17", (many, capi.RF_MAX_PLANES + 1, 0, W, H, 1.0, dx, dy), capi.RF_ERR_INVALID_ARG),
        ("width 0", ([g], 1, 0, 0, H, 1.0, dx, dy), capi.RF_ERR_INVALID_ARG),
        ("height 0", ([g], 1, 0, W, 0, 1.0, dx, dy), capi.RF_ERR_INVALID_ARG),
        ("null guide array", (None, 1, 0, W, H, 1.0, dx, dy), capi.RF_ERR_INVALID_ARG),
        ("null guide plane", ([g, None], 2, 0, W, H, 1.0, dx, dy), capi.RF_ERR_INVALID_ARG),
        ("null dx", ([g], 1, 0, W, H, 1.0, None, dy), capi.RF_ERR_INVALID_ARG),
        ("null dy", ([g], 1, 0, W, H, 1.0, dx, None), capi.RF_ERR_INVALID_ARG),
        ("negative scale", ([g], 1, 0, W, H, -1.0, dx, dy), capi.RF_ERR_INVALID_ARG),
        ("NaN scale", ([g], 1, 0, W, H, float("nan"), dx, dy), capi.RF_ERR_INVALID_ARG),
        ("infinite scale", ([g], 1, 0, W, H, float("inf"), dx, dy), capi.RF_ERR_INVALID_ARG),
        ("dx off by 4 bytes", ([g], 1, 0, W, H, 1.0, dx + 4, dy), capi.RF_ERR_INVALID_ARG),
        ("dy off by 8 bytes", ([g], 1, 0, W, H, 1.0, dx, dy + 8), capi.RF_ERR_INVALID_ARG),
        ("f32 guide off by 4 bytes", ([g + 4], 1, 0, W, H, 1.0, dx, dy), capi.RF_ERR_INVALID_ARG),
        ("uint8 guide off by 2 bytes", ([g + 2], 1, 1, W, H, 1.0, dx, dy), capi.RF_ERR_INVALID_ARG),
        ("dx is dy", ([g], 1, 0, W, H, 1.0, dx, dx), capi.RF_ERR_INVALID_ARG),
        ("dx is the guide", ([g], 1, 0, W, H, 1.0, g, dy), capi.RF_ERR_INVALID_ARG),
        ("dy is the second guide plane", ([g, dy], 2, 0, W, H, 1.0, dx, dy), capi.RF_ERR_INVALID_ARG),
    ]
    for what, args, want in cases:
        status, message = distances(*args)
        assert status == want, f"{what}: status {status} ({message})"
        assert message, f"{what}: no text in rf_last_error_string"
    del keep


def test_distances_overlap_is_by_ranges():
    """dx 16 bytes into dy's plane, and dy inside a uint8 guide's shorter plane"""
    big, at = aligned(3 * PLANE)
    _, g = aligned(PLANE)
    assert distances([g], 1, 0, W, H, 1.0, at, at + PLANE - 16)[0] == capi.RF_ERR_INVALID_ARG
    assert distances([at + PLANE - 16], 1, 1, W, H, 1.0, at, at + 2 * PLANE)[0] == capi.RF_ERR_INVALID_ARG
    del big


# ---- the bases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma_s,K", [(40.0, 3), (60.0, 1), (7.5, 5)])
def test_bases_match_the_closed_form_and_the_weight_planes(sigma_s, K):
    import torch
    bases = rfa.domain_transform_bases(sigma_s, K)
    assert len(bases) == K
    for k, a in enumerate(bases):
        sigma_k = sigma_s * math.sqrt(3.0) * 2.0 ** (K - 1 - k) / math.sqrt(4.0 ** K - 1.0)
        assert a == pytest.approx(math.exp(-math.sqrt(2.0) / sigma_k), rel=1e-15)
        assert 0.0 < a < 1.0
    assert all(a < b for a, b in zip(bases[1:], bases))           # sigma_k halves from one iteration to the next
    # the a_k behind domain_transform_weights: element 0 of a weight line holds a_k ** 1
    weights = rfa.domain_transform_weights(torch.zeros((3, 8, 8)), sigma_s, 0.5, K)
    for (wx, wy), a in zip(weights, bases):
        assert wx.numpy()[0, 0] == np.float32(a) ** np.float32(1) and wy.numpy()[0, 0] == np.float32(a)
    with pytest.raises(ValueError):
        rfa.domain_transform_bases(sigma_s, 0)


# ---- the conversion ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", BASES)
def test_conversion_is_exact_at_zero_and_at_infinity(b):
    l = np.float32(np.log2(np.float64(np.float32(b))))
    assert l.dtype == np.float32 and l < 0
    d = np.array([0.0, np.inf, 1.0], dtype=np.float32)
    w = np.exp2(d * l)
    assert w.dtype == np.float32
    assert w[0] == 1.0 and w[1] == 0.0
    assert abs(float(w[2]) - float(np.float32(b))) <= 2.0 ** -23


# ---- symbols ----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["rf_var_plan_execute_power", "rf_var_plan_execute_power_timed", "rf_var_distances"]


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_symbols_are_exported_and_declared(name):
    assert name in capi.EXPORTED_SYMBOLS
    fn = getattr(capi.lib(), name)                               # resolves in the built library, or raises
    assert fn.argtypes is not None, f"{name} has no argtypes in capi.py"


def test_python_names_are_exported():
    for name in ("domain_transform_bases", "domain_transform_distances", "domain_transform_weights", "edge_aware_smooth", "VarPlan"):
        assert name in rfa.__all__ and hasattr(rfa, name)
    assert hasattr(rfa.VarPlan, "execute_power") and hasattr(rfa.VarPlan, "execute_power_timed")
    assert capi.RF_ABI == 3
