"""CPU tests of the varying scans' adjoint (rf_var_plan_backward): the f64 yardstick against central differences, the tiled f32
algebra (tests/var_grad_emulator.py) under the bar the kernels are held to, the exported surface, and what a host-only plan can
answer: refusals, launch counts, workspace.  No kernel is launched."""
import ctypes

import numpy as np
import pytest

import var_grad_cases as cases
import var_grad_emulator as gemu
import var_grad_loops as loops
import recfilter_amd as rfa
from recfilter_amd import capi

SCAN_LISTS, SHAPES = cases.SCAN_LISTS, cases.SHAPES


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCAN_LISTS))
def test_f64_loops_against_central_differences(name):
    """L = sum(grad_out * out) on 3 x 8, 2 planes: every image sample and every weight the scans read, perturbed by +-h in f64"""
    shape, planes, scans, h = (3, 8), 2, SCAN_LISTS[name], 1e-6
    rng = np.random.default_rng(518)
    ins = [rng.random(shape) * 2 - 1 for _ in range(planes)]
    ws = [rng.random(shape) ** 0.25 for _ in range(2)]
    g = [rng.random(shape) * 2 - 1 for _ in range(planes)]

    def loss(ins_, ws_):
        out = loops.forward(ins_, ws_, scans, np.float64)[-1]
        return sum(float(np.sum(a * b)) for a, b in zip(g, out))

    def poisoned(ws_):      # element 0 is never read: NaN there must reach nothing
        ws_ = [w.copy() for w in ws_]
        ws_[0][:, 0] = np.nan
        ws_[1][0, :] = np.nan
        return ws_
    grad_in, grad_w = loops.backward(ins, poisoned(ws), scans, g, np.float64)
    for pl in range(planes):
        for idx in np.ndindex(shape):
            up, down = [a.copy() for a in ins], [a.copy() for a in ins]
            up[pl][idx] += h
            down[pl][idx] -= h
            num = (loss(up, ws) - loss(down, ws)) / (2 * h)
            assert abs(num - grad_in[pl][idx]) <= 1e-8, (name, "image", pl, idx, num, grad_in[pl][idx])
    read = {k for _, _, k in scans}
    for k in range(2):
        if k not in read:
            assert grad_w[k] is None
            continue
        assert not np.isnan(grad_w[k]).any()
        for idx in np.ndindex(shape):
            if idx[1 - k] == 0:      # element 0 along the scanned dimension (plane 0: x scans, plane 1: y scans)
                assert grad_w[k][idx] == 0.0
                continue
            up, down = [a.copy() for a in ws], [a.copy() for a in ws]
            up[k][idx] += h
            down[k][idx] -= h
            num = (loss(ins, up) - loss(ins, down)) / (2 * h)
            assert abs(num - grad_w[k][idx]) <= 1e-8, (name, "weights", k, idx, num, grad_w[k][idx])


def test_f64_loops_sum_a_plane_read_along_both_dimensions():
    """one weight plane for an x scan and a y scan: the gradient is the sum, against central differences"""
    shape, h = (5, 8), 1e-6
    scans = [(0, True, 0), (1, False, 0)]
    rng = np.random.default_rng(519)
    ins, ws, g = [rng.random(shape) * 2 - 1], [rng.random(shape) ** 0.25], [rng.random(shape) * 2 - 1]
    loss = lambda ws_: float(np.sum(g[0] * loops.forward(ins, ws_, scans, np.float64)[-1][0]))      # noqa: E731
    _, grad_w = loops.backward(ins, ws, scans, g, np.float64)
    for idx in np.ndindex(shape):
        up, down = [ws[0].copy()], [ws[0].copy()]
        up[0][idx] += h
        down[0][idx] -= h
        assert abs((loss(up) - loss(down)) / (2 * h) - grad_w[0][idx]) <= 1e-8, idx


# ---- the tiled algebra in f32, under the bar of the GPU tests, on their shapes -------------------------------------------------
@pytest.mark.parametrize("name", list(SCAN_LISTS))
@pytest.mark.parametrize("shape,planes", SHAPES)
def test_tiled_algebra_under_the_gpu_bar(shape, planes, name):
    ins, ws = cases.case(shape, planes)
    got_in, got_w = gemu.backward(ins, ws, SCAN_LISTS[name], cases.grad_out(shape, planes))
    cases.assert_gradients(got_in, got_w, shape, planes, name, f"emulator {shape} x {planes} {name}")


@pytest.mark.parametrize("name", ["+x-x", "+y-y", "+x-x+y-y"])
def test_tiled_algebra_with_exact_zeros_and_ones(name):
    shape, planes = (70, 260), 1
    ins, ws = cases.case(shape, planes, "sprinkled")
    got_in, got_w = gemu.backward(ins, ws, SCAN_LISTS[name], cases.grad_out(shape, planes))
    cases.assert_gradients(got_in, got_w, shape, planes, name, f"emulator sprinkled {name}", "sprinkled")


# ---- the surface --------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["rf_var_plan_backward", "rf_var_plan_backward_timed", "rf_var_plan_backward_num_kernels", "rf_var_plan_backward_workspace_bytes"]


def test_symbols_are_exported_declared_and_typed():
    L = capi.lib()
    header = open(rfa.capi.CSRC + "/../../include/recfilter_amd.h").read()
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes, f"{name}: no argtypes"
        assert name + "(" in header, f"{name} is not declared in recfilter_amd.h"
    assert L.rf_var_plan_backward_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.rf_var_plan_backward.argtypes) == 7 and len(L.rf_var_plan_backward_timed.argtypes) == 10


def test_python_names_are_exported():
    assert "var_scan" in rfa.__all__ and callable(rfa.var_scan)
    for name in ("backward", "backward_timed", "backward_num_kernels", "backward_workspace_bytes", "apply"):
        assert callable(getattr(rfa.VarPlan, name)), name


def test_abi_revision_is_unchanged():
    assert capi.RF_ABI == 3
    assert b"abi 3" in capi.lib().rf_version()


def test_flags_are_still_refused():
    arr = (capi.VarScanDesc * 1)()
    arr[0].dim, arr[0].causal, arr[0].weights = 0, 1, 0
    d = capi.VarDesc()
    d.ndim, d.abi = 2, capi.RF_ABI
    d.extent[0], d.extent[1] = 64, 64
    d.dtype, d.n_planes, d.n_weights, d.n_scans = capi.RF_F32, 1, 1, 1
    d.scans = ctypes.cast(arr, ctypes.POINTER(capi.VarScanDesc))
    d.device = capi.RF_DEVICE_HOST_ONLY
    for flags in (1, 2, 0x80000000):
        d.flags = flags
        h = ctypes.c_void_p()
        assert capi.lib().rf_var_plan_create(ctypes.byref(d), ctypes.byref(h)) == capi.RF_ERR_INVALID_ARG
        assert b"flags" in capi.lib().rf_last_error_string() and not h.value


# ---- host-only plans ------------------------------------------------------------------------------------------------------------
PX, MX, PY, MY = (0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1)


def host_plan(shape, scans, planes=1, n_weights=2):
    return rfa.VarPlan(shape, scans, planes=planes, n_weights=n_weights, device=capi.RF_DEVICE_HOST_ONLY)


def raw_backward(plan, ins, weights, grad_outs, grad_ins, grad_weights, timed=False):
    """rf_var_plan_backward with arrays of addresses (None: a null array; an address of 0: a null entry); (status, message)"""
    def arr(values):
        return None if values is None else (ctypes.c_void_p * len(values))(*values)
    L = capi.lib()
    args = [plan._h if plan is not None else None, arr(ins), arr(weights), arr(grad_outs), arr(grad_ins), arr(grad_weights), None]
    if timed:
        n = 64
        status = L.rf_var_plan_backward_timed(*args, (ctypes.c_float * n)(), (ctypes.c_char_p * n)(), n)
    else:
        status = L.rf_var_plan_backward(*args)
    return status, L.rf_last_error_string().decode()


A, B, C, D, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000      # 16-byte aligned addresses, never dereferenced: 64 x 64 f32 planes are 0x4000 bytes


@pytest.mark.parametrize("timed", [False, True])
def test_refusals_in_their_order(timed):
    """a host-only plan: what is decided before RF_ERR_HIP comes first, whatever else is wrong with the call"""
    with host_plan((64, 64), [PX, MY]) as plan:
        run = lambda *a: raw_backward(*a, timed=timed)      # noqa: E731
        for args in ((None, [A], [B, C], [D], [E], None), (plan, [A], None, [D], [E], None), (plan, [A], [B, C], None, [E], None),
                     (plan, [A], [B, C], [D], None, None)):
            status, message = run(*args)
            assert status == capi.RF_ERR_INVALID_ARG and "null argument" in message, (status, message)
        status, message = run(plan, None, [B, C], [D], [E], [A, None])
        assert status == capi.RF_ERR_INVALID_ARG and "in_planes" in message, (status, message)
        # in_planes may be null without weight gradients: a null array, or an array of nulls; then the host-only plan is what is refused
        for grad_weights in (None, [None, None]):
            status, message = run(plan, None, [B, C], [D], [E], grad_weights)
            assert status == capi.RF_ERR_HIP and "host-only" in message, (status, message)
        # ... before alignment and overlap are looked at
        status, message = run(plan, [A], [B, C], [D], [D + 4], [B, None])
        assert status == capi.RF_ERR_HIP and "host-only" in message, (status, message)


def test_python_backward_on_a_host_only_plan():
    with host_plan((64, 64), [PX]) as plan:
        with pytest.raises(rfa.RecFilterError) as e:
            plan.backward(None, [], [])
        assert e.value.status == capi.RF_ERR_HIP
        with pytest.raises(rfa.RecFilterError) as e:
            plan.backward_timed([], [], [], None, [None, None])
        assert e.value.status == capi.RF_ERR_HIP


@pytest.mark.parametrize("scans", [[PX], [MX], [PX, MX], [MX, PX], [PX, MX, PY, MY], [PY, PX, MY], [PX, MX, PX]])
@pytest.mark.parametrize("planes", [1, 3])
def test_launch_counts_and_workspace(scans, planes):
    H, W = 96, 132
    with host_plan((H, W), scans, planes=planes) as plan:
        assert plan.backward_num_kernels(False) == 3 * len(scans)
        assert plan.backward_num_kernels(True) == 7 * len(scans)
        assert plan.backward_workspace_bytes(False) == 0
        assert plan.backward_workspace_bytes(True) == (len(scans) + 1) * planes * H * W * 4
        # the forward's figures are what they were: tails (5) and carries (2) per tile, line and plane of the larger dimension
        tiles = lambda n: (n + 63) // 64      # noqa: E731
        slots = max(tiles(W) * H if any(s[0] == 0 for s in scans) else 0, tiles(H) * W if any(s[0] == 1 for s in scans) else 0)
        assert plan.workspace_bytes == slots * 7 * planes * 4
        stages, i = 0, 0
        while i < len(scans):      # runs along one dimension; a run that is exactly {+d, -d} on one weight plane is one stage
            j = i
            while j < len(scans) and scans[j][0] == scans[i][0]:
                j += 1
            stages += 1 if (j - i == 2 and scans[i][1] and not scans[i + 1][1] and scans[i][2] == scans[i + 1][2]) else j - i
            i = j
        assert plan.num_kernels == 3 * stages


def test_timed_capacity_is_checked():
    with host_plan((64, 64), [PX, MX]) as plan:
        L = capi.lib()
        one = (ctypes.c_void_p * 1)(A)
        two = (ctypes.c_void_p * 2)(B, C)
        status = L.rf_var_plan_backward_timed(plan._h, one, two, one, one, None, None, (ctypes.c_float * 5)(), None, 5)
        assert status == capi.RF_ERR_INVALID_ARG and b"need 6" in L.rf_last_error_string()
