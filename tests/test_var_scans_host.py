"""CPU tests of the spatially varying first-order scans: host-only plans (refusals, launch counts, workspace) and the tiling
algebra of kernels_var.hip replayed in numpy f32 (tests/var_scan_emulator.py) against f64 loops.  No kernel is launched."""
import ctypes

import numpy as np
import pytest

import var_scan_emulator as emu
import recfilter_amd as rfa
from recfilter_amd import capi

PX, MX, PY, MY = (0, True), (0, False), (1, True), (1, False)


def with_weights(scans, k=0):
    return [(d, c, k) for d, c in scans]


def host_plan(shape, scans, planes=1, n_weights=1):
    return rfa.VarPlan(shape, scans, planes=planes, n_weights=n_weights, device=capi.RF_DEVICE_HOST_ONLY)


def raw_create(edit, scans=((0, 1, 0),)):
    """rf_var_plan_create on a valid host-only description of a 64 x 64 image after edit(desc); returns (status, message)"""
    arr = (capi.VarScanDesc * len(scans))()
    for i, (dim, causal, weights) in enumerate(scans):
        arr[i].dim, arr[i].causal, arr[i].weights = dim, causal, weights
    d = capi.VarDesc()
    d.ndim, d.abi = 2, capi.RF_ABI
    d.extent[0], d.extent[1] = 64, 64
    d.dtype, d.n_planes, d.n_weights = capi.RF_F32, 1, 1
    d.n_scans, d.scans = len(scans), ctypes.cast(arr, ctypes.POINTER(capi.VarScanDesc))
    d.device, d.flags = capi.RF_DEVICE_HOST_ONLY, 0
    edit(d)
    h = ctypes.c_void_p()
    status = capi.lib().rf_var_plan_create(ctypes.byref(d), ctypes.byref(h))
    message = capi.lib().rf_last_error_string().decode()
    if status == capi.RF_OK:
        capi.lib().rf_var_plan_destroy(h)
    else:
        assert not h.value, "a refused description must not leave a plan behind"
    return status, message


def set_field(name, value):
    def edit(d):
        setattr(d, name, value)
    return edit


def test_valid_description_is_accepted():
    assert raw_create(lambda d: None)[0] == capi.RF_OK


@pytest.mark.parametrize("what,edit,scans,status", [
    ("ndim 1", set_field("ndim", 1), None, capi.RF_ERR_UNSUPPORTED),
    ("ndim 3", set_field("ndim", 3), None, capi.RF_ERR_UNSUPPORTED),
    ("dtype f64", set_field("dtype", capi.RF_F64), None, capi.RF_ERR_UNSUPPORTED),
    ("dtype f16", set_field("dtype", capi.RF_F16), None, capi.RF_ERR_UNSUPPORTED),
    ("abi", set_field("abi", capi.RF_ABI - 1), None, capi.RF_ERR_INVALID_ARG),
    ("n_scans 0", set_field("n_scans", 0), None, capi.RF_ERR_INVALID_ARG),
    ("n_scans 9", None, tuple((0, 1, 0) for _ in range(9)), capi.RF_ERR_INVALID_ARG),
    ("dim -1", None, ((-1, 1, 0),), capi.RF_ERR_INVALID_ARG),
    ("dim 2", None, ((2, 1, 0),), capi.RF_ERR_INVALID_ARG),
    ("weights -1", None, ((0, 1, -1),), capi.RF_ERR_INVALID_ARG),
    ("weights 1 of 1", None, ((0, 1, 1),), capi.RF_ERR_INVALID_ARG),
    ("n_planes 0", set_field("n_planes", 0), None, capi.RF_ERR_INVALID_ARG),
    ("n_planes 17", set_field("n_planes", capi.RF_MAX_PLANES + 1), None, capi.RF_ERR_INVALID_ARG),
    ("flags", set_field("flags", 1), None, capi.RF_ERR_INVALID_ARG),
])
def test_refusals(what, edit, scans, status):
    got, message = raw_create(edit or (lambda d: None), scans or ((0, 1, 0),))
    assert got == status, f"{what}: status {got} ({message})"
    assert message, f"{what}: no text in rf_last_error_string"


@pytest.mark.parametrize("width", [63, 66, 1])
def test_width_must_be_a_multiple_of_four(width):
    with pytest.raises(rfa.RecFilterError) as e:
        host_plan((64, width), with_weights([PX]))
    assert e.value.status == capi.RF_ERR_UNSUPPORTED
    assert "multiple of 4" in str(e.value)


def test_python_plan_refusals():
    with pytest.raises(rfa.RecFilterError) as e:
        host_plan((4, 64, 64), with_weights([PX]))
    assert e.value.status == capi.RF_ERR_UNSUPPORTED
    with pytest.raises(rfa.RecFilterError) as e:
        host_plan((64, 64), [(0, True, 2)], n_weights=2)
    assert e.value.status == capi.RF_ERR_INVALID_ARG


@pytest.mark.parametrize("scans,kernels", [
    (with_weights([PX]), 3), (with_weights([MX]), 3), (with_weights([PY]), 3), (with_weights([MY]), 3),
    (with_weights([PX, MX]), 3),
    (with_weights([MX, PX]), 6),
    (with_weights([PX, MX, PY, MY]), 6),
    (with_weights([PX, MX]) + [(0, True, 1)], 9),
    ([(0, True, 0), (0, False, 1)], 6),              # a pair on two weight planes is two stages
    (with_weights([PX, MY]), 6),                     # ... and so is one across dimensions
])
def test_num_kernels(scans, kernels):
    with host_plan((128, 128), scans, n_weights=2) as plan:
        assert plan.num_kernels == kernels


@pytest.mark.parametrize("planes", [1, 3])
def test_workspace_is_a_fraction_of_the_image(planes):
    with host_plan((1024, 1024), with_weights([PX, MX, PY, MY]), planes=planes) as plan:
        assert 0 < plan.workspace_bytes < planes * 1024 * 1024 * 4 // 4


def test_host_only_plan_refuses_to_execute():
    with host_plan((64, 64), with_weights([PX])) as plan:
        with pytest.raises(rfa.RecFilterError) as e:
            plan.execute([], [], [])
        assert e.value.status == capi.RF_ERR_HIP
        with pytest.raises(rfa.RecFilterError) as e:
            plan.execute_timed([], [], [])
        assert e.value.status == capi.RF_ERR_HIP


def test_abi_revision_is_unchanged():
    assert capi.RF_ABI == 3
    assert b"abi 3" in capi.lib().rf_version()


# ---- the tiling algebra -----------------------------------------------------------------------------------------------------
def dt_weights(rng, lines, n):
    """domain-transform weights a^d of a noisy step signal, a from 0.07 (sigma 0.53) to 0.9993 (sigma 2000), NaN at element 0"""
    g = rng.random((lines, n)) * 0.1 + (np.arange(n) > n // 2)
    d = 1.0 + 8.0 * np.abs(np.diff(g, axis=1, prepend=g[:, :1]))
    a = np.exp(-np.sqrt(2.0) / np.geomspace(0.53, 2000.0, lines))[:, None]
    w = (a ** d).astype(np.float32)
    w[:, 0] = np.nan
    return w


def peak_err(got, want, peak):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want))) / peak


@pytest.mark.parametrize("shape,tile", [((5, 200), 64), ((3, 4096), 32), ((3, 4096), 128)])
@pytest.mark.parametrize("mode,g_form", [(emu.CAUSAL, "sum"), (emu.ANTICAUSAL, "sum"), (emu.PAIR, "sum"), (emu.PAIR, "scan")])
def test_tiled_algebra_against_f64_loops(shape, tile, mode, g_form):
    """The bar of the GPU tests: max abs error over the input peak <= max(4 x the f32 serial loop's, 1e-6).  (G belongs to
    the pair: its two forms run there.)"""
    rng = np.random.default_rng(1511)
    x = (rng.random(shape) * 2 - 1).astype(np.float32)
    w = dt_weights(rng, *shape)

    def run(fn_serial, dtype):
        v = x
        if mode != emu.ANTICAUSAL:
            v = fn_serial(v, w, True, dtype)
        if mode != emu.CAUSAL:
            v = fn_serial(v, w, False, dtype)
        return v
    want = run(emu.serial, np.float64)
    peak = float(np.max(np.abs(x)))
    serial32 = peak_err(run(emu.serial, np.float32), want, peak)
    got = emu.tiled_stage(x, w, mode, tile, g_form)
    assert not np.isnan(got).any(), "the NaN at element 0 of the weights reached the output"
    err = peak_err(got, want, peak)
    assert err <= max(4 * serial32, 1e-6), f"tiled {err:.3e} against the f32 serial loop's {serial32:.3e}"


@pytest.mark.parametrize("mode,expect", [(emu.CAUSAL, "first"), (emu.ANTICAUSAL, "last"), (emu.PAIR, "first")])
def test_tiled_algebra_is_exact_for_weights_of_one(mode, expect):
    rng = np.random.default_rng(7)
    x = (rng.random((4, 200)) * 2 - 1).astype(np.float32)
    got = emu.tiled_stage(x, np.ones_like(x), mode, 64)
    np.testing.assert_array_equal(got, np.repeat(x[:, :1] if expect == "first" else x[:, -1:], 200, axis=1))
    np.testing.assert_array_equal(emu.tiled_stage(x, np.zeros_like(x), mode, 64), x)
