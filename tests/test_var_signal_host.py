"""CPU tests of the varying scans on long 1-D signals (rf_var_plan_create_signal): host-only plans -- creation, launch counts,
the workspace, every refusal with its status and text -- and the two-level tiling of kernels_var_signal.hip replayed in numpy f32
(tests/var_signal_emulator.py) against f64 loops; the gradient loops the GPU tests use, pinned on a signal by central differences.
No kernel is launched."""
import ctypes

import numpy as np
import pytest

import var_signal_emulator as emu
import recfilter_amd as rfa
from recfilter_amd import capi

P, M = (0, True, 0), (0, False, 0)
SCAN_LISTS = {"+x": [P], "-x": [M], "+x-x": [P, M], "-x+x": [M, P], "+x-x+x": [P, M, P], "+x-x two weights": [(0, True, 0), (0, False, 1)]}
STAGES = {"+x": 1, "-x": 1, "+x-x": 1, "-x+x": 2, "+x-x+x": 3, "+x-x two weights": 2}


def host_plan(length, scans, planes=1, n_weights=2):
    return rfa.VarPlan.signal(length, scans, planes=planes, n_weights=n_weights, device=capi.RF_DEVICE_HOST_ONLY)


def raw_create(edit, scans=((0, 1, 0),)):
    """rf_var_plan_create_signal on a valid host-only description of 4096 samples after edit(desc); returns (status, message)"""
    arr = (capi.VarScanDesc * len(scans))()
    for i, (dim, causal, weights) in enumerate(scans):
        arr[i].dim, arr[i].causal, arr[i].weights = dim, causal, weights
    d = capi.VarSignalDesc()
    d.abi, d.length, d.dtype = capi.RF_ABI, 4096, capi.RF_F32
    d.n_planes, d.n_weights = 1, 1
    d.n_scans, d.scans = len(scans), ctypes.cast(arr, ctypes.POINTER(capi.VarScanDesc))
    d.device, d.flags = capi.RF_DEVICE_HOST_ONLY, 0
    edit(d)
    h = ctypes.c_void_p()
    status = capi.lib().rf_var_plan_create_signal(ctypes.byref(d), ctypes.byref(h))
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


# ---- host-only plans ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [4, 64, 4096, 10_000_000, 1 << 30])
def test_valid_description_is_accepted(length):
    assert raw_create(set_field("length", length))[0] == capi.RF_OK


@pytest.mark.parametrize("what,edit,scans,status,text", [
    ("length 6", set_field("length", 6), None, capi.RF_ERR_UNSUPPORTED, "length"),
    ("length 4099", set_field("length", 4099), None, capi.RF_ERR_UNSUPPORTED, "length"),
    ("length 2^30 + 4", set_field("length", (1 << 30) + 4), None, capi.RF_ERR_UNSUPPORTED, "length"),
    ("length 0", set_field("length", 0), None, capi.RF_ERR_INVALID_ARG, "length"),
    ("dtype f64", set_field("dtype", capi.RF_F64), None, capi.RF_ERR_UNSUPPORTED, "dtype"),
    ("dtype f16", set_field("dtype", capi.RF_F16), None, capi.RF_ERR_UNSUPPORTED, "dtype"),
    ("dim 1", None, ((1, 1, 0),), capi.RF_ERR_INVALID_ARG, "dim"),
    ("dim -1", None, ((-1, 1, 0),), capi.RF_ERR_INVALID_ARG, "dim"),
    ("abi", set_field("abi", capi.RF_ABI - 1), None, capi.RF_ERR_INVALID_ARG, "abi"),
    ("n_scans 0", set_field("n_scans", 0), None, capi.RF_ERR_INVALID_ARG, "n_scans"),
    ("n_scans 9", None, tuple((0, 1, 0) for _ in range(9)), capi.RF_ERR_INVALID_ARG, "n_scans"),
    ("n_planes 0", set_field("n_planes", 0), None, capi.RF_ERR_INVALID_ARG, "n_planes"),
    ("n_planes 17", set_field("n_planes", capi.RF_MAX_PLANES + 1), None, capi.RF_ERR_INVALID_ARG, "n_planes"),
    ("n_weights 0", set_field("n_weights", 0), None, capi.RF_ERR_INVALID_ARG, "n_weights"),
    ("n_weights 9", set_field("n_weights", capi.RF_VAR_MAX_SCANS + 1), None, capi.RF_ERR_INVALID_ARG, "n_weights"),
    ("weights 1 of 1", None, ((0, 1, 1),), capi.RF_ERR_INVALID_ARG, "weights"),
    ("flags", set_field("flags", 1), None, capi.RF_ERR_INVALID_ARG, "flags"),
])
def test_refusals(what, edit, scans, status, text):
    got, message = raw_create(edit or (lambda d: None), scans or ((0, 1, 0),))
    assert got == status, f"{what}: status {got} ({message})"
    assert text in message, f"{what}: the message does not name the field: {message!r}"


def test_the_image_entry_point_still_refuses_one_dimension():
    with pytest.raises(rfa.RecFilterError) as e:
        rfa.VarPlan((4096,), [P], device=capi.RF_DEVICE_HOST_ONLY)
    assert e.value.status == capi.RF_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", list(SCAN_LISTS))
def test_num_kernels(name):
    with host_plan(12616, SCAN_LISTS[name]) as plan:
        assert plan.shape == (12616,)
        assert plan.num_kernels == 3 * STAGES[name]
        n = len(SCAN_LISTS[name])
        assert plan.backward_num_kernels(False) == 3 * n
        assert plan.backward_num_kernels(True) == 7 * n


@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("length", [4096, 4100, 12616, 10_000_000, 1 << 30])
def test_workspace_is_the_exact_sum_and_a_fraction_of_the_signals(length, planes):
    tiles = -(-length // 64)
    groups = -(-tiles // 64)
    with host_plan(length, [P, M], planes=planes) as plan:
        assert plan.workspace_bytes == 4 * planes * (5 * (tiles + groups) + 2 * groups)
        assert plan.workspace_bytes < planes * length * 4 // 8      # from one full group on
        assert plan.backward_workspace_bytes(True) == 3 * planes * length * 4
        assert plan.backward_workspace_bytes(False) == 0


def test_host_only_plan_refuses_to_run():
    with host_plan(4096, [P, M]) as plan:
        for call in (lambda: plan.execute([], [], []), lambda: plan.execute_timed([], [], []),
                     lambda: plan.execute_power([], [], [0.5, 0.5], []), lambda: plan.backward(None, [], [], None, None),
                     lambda: plan.backward_power(None, [], [0.5, 0.5], [], None, None)):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == capi.RF_ERR_HIP


def test_abi_revision_is_unchanged():
    assert capi.RF_ABI == 3
    assert b"abi 3" in capi.lib().rf_version()
    assert "rf_var_plan_create_signal" in capi.EXPORTED_SYMBOLS


# ---- the two-level tiling -------------------------------------------------------------------------------------------------------
def weights_of(kind, rng, n):
    w = (rng.random(n) ** 0.25 if kind == "quarter" else 0.99 + 0.01 * rng.random(n)).astype(np.float32)
    w = np.minimum(w, np.float32(1) - np.float32(2.0 ** -24)) if kind == "near one" else w
    w[0] = np.nan
    return w


@pytest.mark.parametrize("kind", ["quarter", "near one"])
@pytest.mark.parametrize("mode", [emu.CAUSAL, emu.ANTICAUSAL, emu.PAIR])
@pytest.mark.parametrize("n", [4, 64, 68, 4096, 4100, 12616])
def test_two_level_scheme_against_f64_loops(n, mode, kind):
    """The bar of the GPU tests: max abs error over the input peak <= max(4 x the f32 serial loop's, 1e-6)."""
    rng = np.random.default_rng(1000 * n + 10 * mode + len(kind))
    x = (rng.random(n) * 2 - 1).astype(np.float32)
    w = weights_of(kind, rng, n)
    want = emu.serial_stage(x, w, mode, np.float64)
    peak = float(np.max(np.abs(x)))
    err32 = float(np.max(np.abs(emu.serial_stage(x, w, mode, np.float32).astype(np.float64) - want))) / peak
    got = emu.tiled_stage(x, w, mode)
    assert not np.isnan(got).any(), "the NaN at element 0 of the weights reached the output"
    err = float(np.max(np.abs(got.astype(np.float64) - want))) / peak
    print(f"n {n} mode {mode} {kind}: two-level {err:.3e}, f32 serial loop {err32:.3e}")
    assert err <= max(4 * err32, 1e-6), f"two-level {err:.3e} against the f32 serial loop's {err32:.3e}"


def test_composition_is_associative():
    """(A B) C against A (B C) in f32, both against the f64 value: the difference is rounding, a few ulps of the terms' sizes"""
    rng = np.random.default_rng(5)
    n = 4096

    def tuples(dtype):
        return [tuple(a.astype(dtype) for a in t) for t in raw]
    raw = [(rng.random(n) * 2 - 1, rng.random(n), rng.random(n) * 2 - 1, rng.random(n), rng.random(n)) for _ in range(3)]
    A, B, C = tuples(np.float64)
    left, right = emu.compose(emu.compose(A, B), C), emu.compose(A, emu.compose(B, C))
    for l, r in zip(left, right):
        np.testing.assert_allclose(l, r, rtol=0, atol=1e-14)
    a, b, c = tuples(np.float32)
    for got in (emu.compose(emu.compose(a, b), c), emu.compose(a, emu.compose(b, c))):
        for g, want in zip(got, left):
            assert g.dtype == np.float32
            # every component is a sum of at most 4 products of values in [-1, 1]: magnitudes below 4, a handful of roundings
            np.testing.assert_allclose(g, want, rtol=0, atol=16 * 2.0 ** -24 * 4)
    # the identity, on both sides, exactly
    e = emu.identity((n,))
    for got in (emu.compose(e, a), emu.compose(a, e)):
        for g, want in zip(got, a):
            np.testing.assert_array_equal(g, want)


@pytest.mark.parametrize("mode,expect", [(emu.CAUSAL, "first"), (emu.ANTICAUSAL, "last"), (emu.PAIR, "first")])
@pytest.mark.parametrize("n", [68, 4100, 12616])
def test_weights_of_zero_and_one_are_exact(n, mode, expect):
    rng = np.random.default_rng(n)
    x = (rng.random(n) * 2 - 1).astype(np.float32)
    np.testing.assert_array_equal(emu.tiled_stage(x, np.zeros(n, np.float32), mode), x)
    got = emu.tiled_stage(x, np.ones(n, np.float32), mode)
    np.testing.assert_array_equal(got, np.full(n, x[0] if expect == "first" else x[-1]))


# ---- the gradient loops on a signal ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["+x-x", "-x+x", "+x-x two weights"])
def test_gradient_loops_against_central_differences(name):
    """tests/var_grad_loops.py and tests/smooth_grad_loops.py, the yardsticks of the GPU tests, on a (1, 68) signal in f64: the
    directional derivative of L = sum(g * out) along random directions in x, in the weights and in the exponents"""
    import smooth_grad_loops as power_loops
    import var_grad_loops as loops
    n, scans, h = 68, SCAN_LISTS[name], 1e-6
    rng = np.random.default_rng(68)
    x, g, dx = (rng.random((1, n)) * 2 - 1 for _ in range(3))
    ws = [rng.random((1, n)) * 0.9 + 0.05 for _ in range(2)]
    ds = [1 + 3 * rng.random((1, n)) for _ in range(2)]
    dws = [rng.random((1, n)) * 2 - 1 for _ in range(2)]
    bases = [0.8, 0.97]
    used = sorted({k for _, _, k in scans})

    def loss(xx, weights):
        return float(np.sum(g * loops.forward([xx], weights, scans, np.float64)[-1][0]))

    def shifted(planes, t):
        return [p + t * d for p, d in zip(planes, dws)]
    gin, gw = loops.backward([x], ws, scans, [g], np.float64)
    assert abs((loss(x + h * dx, ws) - loss(x - h * dx, ws)) / (2 * h) - float(np.sum(gin[0] * dx))) < 1e-7
    numeric = (loss(x, shifted(ws, h)) - loss(x, shifted(ws, -h))) / (2 * h)
    assert abs(numeric - sum(float(np.sum(gw[k][:, 1:] * dws[k][:, 1:])) for k in used)) < 1e-7
    assert all(np.all(gw[k][:, 0] == 0) for k in used)

    def power(planes):
        return [np.exp2(d * np.log2(np.float64(np.float32(b)))) for d, b in zip(planes, bases)]
    _, gd = power_loops.power_backward([x], ds, bases, scans, [g], np.float64)
    numeric = (loss(x, power(shifted(ds, h))) - loss(x, power(shifted(ds, -h)))) / (2 * h)
    assert abs(numeric - sum(float(np.sum(gd[k][:, 1:] * dws[k][:, 1:])) for k in used)) < 1e-7
