"""CPU tests of the differentiable smoothing plan (rf_var_plan_backward_power, rf_var_distances_backward, rf_smooth_plan_backward):
the f64 yardstick of tests/smooth_grad_loops.py against central differences and against torch's autograd, the f32 loops under the
bar the kernels are held to, the exported surface, and what host-only plans and calls without a device can answer: refusals in
their order, launch counts, workspace.  No kernel is launched."""
import ctypes

import numpy as np
import pytest

import smooth_cases as sc
import smooth_grad_cases as cases
import smooth_grad_loops as sloops
import var_grad_cases as vcases
import recfilter_amd as rfa
from recfilter_amd import capi

ALL = vcases.SCAN_LISTS["+x-x+y-y"]


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
def tiny():
    """(2, 6, 8), K = 2: image, a guide whose neighbours differ by far more than the step, grad_out, bases, scale"""
    shape, K = (2, 6, 8), 2
    rng = np.random.default_rng(1519)
    image = rng.random(shape) * 2 - 1
    guide = 0.5 * rng.random(shape) + np.linspace(0, 2, 8)[None, None, :] + np.linspace(0, 2, 6)[None, :, None]
    smallest = min(np.abs(np.diff(guide, axis=2)).min(), np.abs(np.diff(guide, axis=1)).min())
    assert smallest > 1e-3, smallest      # the step below is 1e-6
    g = rng.random(shape) * 2 - 1
    return image, guide, g, [float(a) for a in sc.bases_f32(3.0, K)], 3.0 / 0.8


H_STEP, TOL = 1e-6, 1e-8      # the step and the tolerance of tests/test_var_grad_host.py, the tolerance relative to a peak of >= 1


def central(loss, x, idx):
    up, down = x.copy(), x.copy()
    up[idx] += H_STEP
    down[idx] -= H_STEP
    return (loss(up) - loss(down)) / (2 * H_STEP)


def test_f64_power_backward_against_central_differences():
    """L = sum(grad_out * out) of +x -x +y -y in the power form: every image sample and every exponent"""
    image, guide, g, _, scale = tiny()
    d = sloops.distances(guide, scale, np.float64)
    bases = [0.9, 0.8]

    def loss(planes, ds):
        ws = [sloops.power_weights(e, a, np.float64) for e, a in zip(ds, bases)]
        out = sloops.loops.forward(planes, ws, ALL, np.float64)[-1]
        return sum(float(np.sum(a * b)) for a, b in zip(g, out))
    poisoned = [d[0].copy(), d[1].copy()]      # element 0 is never read: NaN there must reach nothing
    poisoned[0][:, 0] = np.nan
    poisoned[1][0, :] = np.nan
    grad_in, grad_d = sloops.power_backward(list(image), poisoned, bases, ALL, list(g), np.float64)
    for pl in range(2):
        for idx in np.ndindex(image.shape[1:]):
            num = central(lambda v: loss([v if q == pl else image[q] for q in range(2)], d), image[pl], idx)
            assert abs(num - grad_in[pl][idx]) <= TOL, ("image", pl, idx, num, grad_in[pl][idx])
    for k in range(2):
        assert not np.isnan(grad_d[k]).any()
        peak = max(1.0, float(np.abs(grad_d[k]).max()))
        for idx in np.ndindex(d[k].shape):
            if idx[1 - k] == 0:
                assert grad_d[k][idx] == 0.0
                continue
            num = central(lambda v: loss(list(image), [v if q == k else d[q] for q in range(2)]), d[k], idx)
            assert abs(num - grad_d[k][idx]) <= TOL * peak, ("exponent", k, idx, num, grad_d[k][idx])


def test_f64_distances_backward_against_central_differences():
    image, guide, g, _, scale = tiny()
    rng = np.random.default_rng(1520)
    gdx, gdy = rng.random(guide.shape[1:]) * 2 - 1, rng.random(guide.shape[1:]) * 2 - 1

    def loss(gd):
        dx, dy = sloops.distances(gd, scale, np.float64)
        return float(np.sum(gdx * dx) + np.sum(gdy * dy))
    got = sloops.distances_backward(guide, scale, gdx, gdy, np.float64)
    peak = max(1.0, float(np.abs(got).max()))
    for idx in np.ndindex(guide.shape):
        num = central(loss, guide, idx)
        assert abs(num - got[idx]) <= TOL * peak, (idx, num, got[idx])


@pytest.mark.parametrize("self_guided", [False, True])
def test_f64_filter_backward_against_central_differences(self_guided):
    """the whole filter, K = 2, through the distances: image and guide gradients (one gradient where the image guides itself)"""
    image, guide, g, bases, scale = tiny()
    if self_guided:      # the image must have no ties of its own
        image = guide - 2.0
        guide = None

    def loss(im, gd):
        ds = sloops.distances(im if gd is None else gd, scale, np.float64)
        return float(np.sum(g * np.stack(sloops.smooth_forward(im, ds, bases, np.float64)[-1])))
    grad_image, grad_guide, _ = sloops.smooth_backward(image, guide, bases, scale, g, np.float64, True)
    peak = max(1.0, float(np.abs(grad_image).max()))
    for idx in np.ndindex(image.shape):
        num = central(lambda v: loss(v, guide), image, idx)
        assert abs(num - grad_image[idx]) <= TOL * peak, ("image", idx, num, grad_image[idx])
    if not self_guided:
        peak = max(1.0, float(np.abs(grad_guide).max()))
        for idx in np.ndindex(guide.shape):
            num = central(lambda v: loss(image, v), guide, idx)
            assert abs(num - grad_guide[idx]) <= TOL * peak, ("guide", idx, num, grad_guide[idx])
        # with the distances held constant the image gradient is the same and there is no guide gradient
        held = sloops.smooth_backward(image, guide, bases, scale, g, np.float64, False)
        assert np.array_equal(held[0], grad_image) and held[1] is None


@pytest.mark.parametrize("self_guided", [False, True])
def test_f64_loops_agree_with_torch_autograd(self_guided):
    import torch
    image, guide, g, bases, scale = tiny()
    if self_guided:
        image, guide = guide - 2.0, None
    im = torch.from_numpy(image).requires_grad_(True)
    gd = None if guide is None else torch.from_numpy(guide).requires_grad_(True)
    sloops.torch_filter(im, gd, bases, scale, torch.float64).backward(torch.from_numpy(g))
    grad_image, grad_guide, _ = sloops.smooth_backward(image, guide, bases, scale, g, np.float64, True)
    assert np.max(np.abs(im.grad.numpy() - grad_image)) <= 1e-12 * max(1.0, np.abs(grad_image).max())
    if not self_guided:
        assert np.max(np.abs(gd.grad.numpy() - grad_guide)) <= 1e-12 * max(1.0, np.abs(grad_guide).max())


@pytest.mark.parametrize("shape,K", cases.CASES)
@pytest.mark.parametrize("self_guided", [False, True])
def test_f32_loops_pass_the_bar_in_either_order_of_accumulation(shape, K, self_guided):
    """the bar is one the reference itself passes on these inputs: the f32 loops with gd_x, gd_y summed in the plan's order
    (k = K-1 first) define it, and the same loops summing k = 0 first stay under it"""
    want_im, want_gd, err_im, err_gd = cases.expected(shape, K, self_guided, True)
    gd = None if self_guided else cases.guide(shape)
    for order in ("plan", "forward"):
        got = sloops.smooth_backward(cases.image(shape), gd, cases.bases(K), cases.SCALE, cases.grad_out(shape), np.float32, True, order)
        cases.assert_under_bar([got[0]], [want_im], err_im, f"f32 loops {shape} K={K} {order} image")
        if not self_guided:
            cases.assert_under_bar([got[1]], [want_gd], err_gd, f"f32 loops {shape} K={K} {order} guide")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_constant_guide_gets_a_gradient_of_exactly_zero(dtype):
    shape = (3, 130, 132)
    guide = np.full(shape, 0.375, dtype=np.float32)
    got = sloops.smooth_backward(cases.image(shape), guide, cases.bases(2), cases.SCALE, cases.grad_out(shape), dtype, True)
    assert np.abs(got[2][0]).max() > 0 and np.array_equal(got[1], np.zeros(shape, dtype=dtype))


# ---- the exported surface -------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["rf_var_plan_backward_power", "rf_var_plan_backward_power_timed", "rf_var_distances_backward", "rf_smooth_plan_backward",
               "rf_smooth_plan_backward_timed", "rf_smooth_plan_backward_num_kernels", "rf_smooth_plan_backward_workspace_bytes"]


def test_symbols_are_exported_declared_and_typed():
    L = capi.lib()
    header = open(rfa.capi.CSRC + "/../../include/recfilter_amd.h").read()
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes, f"{name}: no argtypes"
        assert name + "(" in header, f"{name} is not declared in recfilter_amd.h"
    assert L.rf_smooth_plan_backward_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.rf_var_plan_backward_power.argtypes) == 8 and len(L.rf_var_plan_backward_power_timed.argtypes) == 11
    assert len(L.rf_var_distances_backward.argtypes) == 11
    assert len(L.rf_smooth_plan_backward.argtypes) == 8 and len(L.rf_smooth_plan_backward_timed.argtypes) == 11


def test_python_names_are_exported():
    assert "domain_transform_distances_backward" in rfa.__all__
    for name in ("backward_power", "backward_power_timed", "apply_power"):
        assert callable(getattr(rfa.VarPlan, name)), name
    for name in ("backward", "backward_timed", "backward_num_kernels", "backward_workspace_bytes", "apply"):
        assert callable(getattr(rfa.SmoothPlan, name)), name


def test_abi_revision_is_unchanged():
    assert capi.RF_ABI == 3
    assert b"abi 3" in capi.lib().rf_version()


def test_differentiable_power_form_is_refused_by_name():
    with pytest.raises(ValueError, match="plan"):
        rfa.edge_aware_smooth(None, form="power", differentiable=True)


# ---- host-only plans and calls without a device -----------------------------------------------------------------------------
A, B, C, D, E, F = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000      # 16-byte aligned, never dereferenced; 64 x 64 f32: 0x4000 bytes


def arr(values):
    return None if values is None else (ctypes.c_void_p * len(values))(*values)


def message():
    return capi.lib().rf_last_error_string().decode()


def raw_power(plan, ins, exponents, bases, grad_outs, grad_ins, grad_exponents, timed=False):
    L = capi.lib()
    pb = None if bases is None else (ctypes.c_float * len(bases))(*bases)
    args = [plan._h if plan is not None else None, arr(ins), arr(exponents), pb, arr(grad_outs), arr(grad_ins), arr(grad_exponents), None]
    if timed:
        status = L.rf_var_plan_backward_power_timed(*args, (ctypes.c_float * 64)(), (ctypes.c_char_p * 64)(), 64)
    else:
        status = L.rf_var_plan_backward_power(*args)
    return status, message()


@pytest.mark.parametrize("timed", [False, True])
def test_power_backward_refusals_in_their_order(timed):
    """those of rf_var_plan_backward, the base check directly before the host-only one"""
    with rfa.VarPlan((64, 64), [(0, True, 0), (1, False, 1)], planes=1, n_weights=2, device=capi.RF_DEVICE_HOST_ONLY) as plan:
        run = lambda *a: raw_power(*a, timed=timed)      # noqa: E731
        ok = [0.5, 0.5]
        for args in ((None, [A], [B, C], ok, [D], [E], None), (plan, [A], None, ok, [D], [E], None), (plan, [A], [B, C], None, [D], [E], None),
                     (plan, [A], [B, C], ok, None, [E], None), (plan, [A], [B, C], ok, [D], None, None)):
            status, text = run(*args)
            assert status == capi.RF_ERR_INVALID_ARG and "null argument" in text, (status, text)
        # exponent gradients without the input planes come before a bad base
        status, text = run(plan, None, [B, C], [0.5, 1.0], [D], [E], [A, None])
        assert status == capi.RF_ERR_INVALID_ARG and "in_planes" in text, (status, text)
        for bad in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
            status, text = run(plan, [A], [B, C], [0.5, bad], [D], [E], None)
            assert status == capi.RF_ERR_INVALID_ARG and "exponent plane 1" in text and "(0, 1)" in text, (bad, status, text)
        # then the host-only plan, before alignment and overlap are looked at
        for grad_exponents in (None, [None, None], [F, None]):
            status, text = run(plan, [A], [B, C], ok, [D], [D + 4], grad_exponents)
            assert status == capi.RF_ERR_HIP and "host-only" in text, (status, text)
        # one plan runs either form: the plane form's entry still answers
        assert capi.lib().rf_var_plan_backward(plan._h, arr([A]), arr([B, C]), arr([D]), arr([E]), None, None) == capi.RF_ERR_HIP
        assert plan.backward_num_kernels(False) == 6 and plan.backward_num_kernels(True) == 14


def test_python_power_backward_on_a_host_only_plan():
    with rfa.VarPlan((64, 64), [(0, True, 0)], planes=1, n_weights=1, device=capi.RF_DEVICE_HOST_ONLY) as plan:
        with pytest.raises(rfa.RecFilterError) as e:
            plan.backward_power(None, [], [0.5], [])
        assert e.value.status == capi.RF_ERR_HIP
        with pytest.raises(rfa.RecFilterError) as e:
            plan.backward_power_timed([], [], [2.0], [], None, [None])
        assert e.value.status == capi.RF_ERR_INVALID_ARG and "(0, 1)" in str(e.value)


def raw_distances_backward(guide, n_guide, width, height, scale, gdx, gdy, grads, accumulate=0):
    status = capi.lib().rf_var_distances_backward(arr(guide), n_guide, width, height, scale, gdx, gdy, arr(grads), accumulate, -1, None)
    return status, message()


def test_distances_backward_refusals_are_decided_without_a_device():
    """every refusal, in order: each call is wrong in the way named and in everything that is checked later"""
    INV, UNS = capi.RF_ERR_INVALID_ARG, capi.RF_ERR_UNSUPPORTED
    run = raw_distances_backward
    for n in (0, capi.RF_MAX_PLANES + 1):
        assert run(None, n, 0, 0, -1.0, None, None, None)[0] == INV and "n_guide" in message()
    assert run(None, 1, 0, 64, -1.0, None, None, None)[0] == INV and "positive" in message()
    for args in ((None, B, C, [D]), ([A], None, C, [D]), ([A], B, None, [D]), ([A], B, C, None)):
        assert run(args[0], 1, 62, 64, -1.0, args[1], args[2], args[3])[0] == INV and "null argument" in message()
    for guide, grads in (([A, None], [D, E]), ([A, F], [D, None])):
        assert run(guide, 2, 62, 64, -1.0, B, C, grads)[0] == INV and "guide plane 1: null pointer" in message()
    for scale in (-1.0, float("nan"), float("inf")):
        assert run([A], 1, 62, 64, scale, B, C, [D], 2)[0] == INV and "scale" in message()
    assert run([A], 1, 62, 64, 1.0, B, C, [D], 2)[0] == INV and "accumulate" in message()
    assert run([A], 1, 62, 64, 1.0, B + 4, C, [D])[0] == UNS and "multiple of 4" in message()
    assert run([A], 1, 64, (1 << 21) + 1, 1.0, B + 4, C, [D])[0] == UNS and "above" in message()
    assert run([A + 4], 1, 64, 64, 1.0, B + 4, C, [D])[0] == INV and "grad_dx and grad_dy" in message()
    for guide, grads in (([A + 4], [B]), ([A], [B + 8])):
        assert run(guide, 1, 64, 64, 1.0, B, C, grads)[0] == INV and "guide plane 0" in message() and "16-byte" in message()
    # overlaps: 64 x 64 f32 planes are 0x4000 bytes
    assert run([A], 1, 64, 64, 1.0, B, C, [B + 0x3ff0])[0] == INV and "gradient of guide plane 0 overlaps grad_dx or grad_dy" in message()
    assert run([A], 1, 64, 64, 1.0, B, C, [C])[0] == INV and "grad_dx or grad_dy" in message()
    assert run([A, D], 2, 64, 64, 1.0, B, C, [E, D + 0x1000])[0] == INV and "gradient of guide plane 1 overlaps guide plane 1" in message()
    assert run([A, D], 2, 64, 64, 1.0, B, C, [E, A])[0] == INV and "gradient of guide plane 1 overlaps guide plane 0" in message()
    assert run([A, D], 2, 64, 64, 1.0, B, C, [E, E + 0x100])[0] == INV and "gradient of guide plane 0 overlaps gradient of guide plane 1" in message()


def host_smooth(shape=(64, 64), planes=1, guide_planes=0, K=2, image_dtype=None, guide_dtype=None):
    return rfa.SmoothPlan(shape, planes=planes, guide_planes=guide_planes, image_dtype=image_dtype, guide_dtype=guide_dtype, iterations=K,
                          sigma_s=cases.SIGMA_S, sigma_r=cases.SIGMA_R, device=capi.RF_DEVICE_HOST_ONLY)


def raw_smooth(plan, image, guide, grad_out, grad_image, grad_guide, edges, timed=False):
    L = capi.lib()
    args = [plan._h if plan is not None else None, arr(image), arr(guide), arr(grad_out), arr(grad_image), arr(grad_guide), edges, None]
    if timed:
        status = L.rf_smooth_plan_backward_timed(*args, (ctypes.c_float * 512)(), (ctypes.c_char_p * 512)(), 512)
    else:
        status = L.rf_smooth_plan_backward(*args)
    return status, message()


@pytest.mark.parametrize("timed", [False, True])
def test_smooth_backward_refusals_in_their_order(timed):
    import torch
    INV, UNS, HIP = capi.RF_ERR_INVALID_ARG, capi.RF_ERR_UNSUPPORTED, capi.RF_ERR_HIP
    run = lambda *a: raw_smooth(*a, timed=timed)      # noqa: E731
    with host_smooth(guide_planes=1) as plan, host_smooth() as self_plan, host_smooth(image_dtype=torch.uint8) as byte_plan, \
            host_smooth(guide_planes=1, guide_dtype=torch.uint8) as byte_guide_plan:
        for args in ((None, [A], [B], [C], [D], [E], 1), (plan, [A], [B], None, [D], [E], 1), (plan, [A], [B], [C], None, [E], 1)):
            status, text = run(*args)
            assert status == INV and "null argument" in text, (status, text)
        for edges in (-1, 2):
            status, text = run(byte_plan, None, [B], [C], [D], [E], edges)
            assert status == INV and "edges must be 0 or 1" in text, (status, text)
        # a byte-image plan, whatever else is wrong
        for edges in (0, 1):
            status, text = run(byte_plan, None, [B], [C], [D], [E], edges)
            assert status == UNS and "uint8" in text, (status, text)
        status, text = run(plan, None, None, [C], [D], None, 1)
        assert status == INV and "guide_planes is null" in text, (status, text)
        status, text = run(self_plan, None, [B], [C], [D], [E], 1)
        assert status == INV and "guide_planes must be null" in text, (status, text)
        # the image planes: needed through the distances, and where the image guides itself
        status, text = run(plan, None, [B], [C], [D], None, 1)
        assert status == INV and "image_planes is null" in text, (status, text)
        status, text = run(self_plan, None, None, [C], [D], [E], 0)
        assert status == INV and "image_planes is null" in text, (status, text)
        # a byte guide: refused only through the distances
        status, text = run(byte_guide_plan, [A], [B], [C], [D], None, 1)
        assert status == UNS and "uint8 guide" in text, (status, text)
        status, text = run(byte_guide_plan, None, [B], [C], [D], None, 0)
        assert status == HIP and "host-only" in text, (status, text)
        # the guide's gradient planes: required with a separate guide through the distances, refused everywhere else
        status, text = run(plan, [A], [B], [C], [D], None, 1)
        assert status == INV and "grad_guide_planes is null" in text, (status, text)
        status, text = run(plan, [A], [B], [C], [D], [E], 0)
        assert status == INV and "grad_guide_planes must be null" in text, (status, text)
        status, text = run(self_plan, [A], None, [C], [D], [E], 1)
        assert status == INV and "grad_guide_planes must be null" in text, (status, text)
        # then the host-only plan, before alignment and overlap are looked at
        for p, args in ((plan, ([A], [B], [C], [C + 4], [A], 1)), (plan, (None, [B], [C], [C + 4], None, 0)),
                        (self_plan, ([A], None, [C], [A], None, 1)), (self_plan, ([A], None, [C], [A], None, 0))):
            status, text = run(p, *args)
            assert status == HIP and "host-only" in text, (status, text)


def test_python_smooth_backward_on_host_only_plans():
    import torch
    with host_smooth(guide_planes=1) as plan:
        with pytest.raises(rfa.RecFilterError) as e:
            plan.backward([], [], [], edges=False)
        assert e.value.status == capi.RF_ERR_HIP
    with host_smooth(image_dtype=torch.uint8) as plan:
        with pytest.raises(rfa.RecFilterError) as e:
            plan.backward_timed([], None, [], edges=True)
        assert e.value.status == capi.RF_ERR_UNSUPPORTED


@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("planes,guide_planes", [(1, 0), (3, 0), (3, 1), (2, 3)])
def test_smooth_launch_counts_and_workspace(K, planes, guide_planes):
    H, W = 96, 132
    with host_smooth((H, W), planes, guide_planes, K) as plan:
        assert plan.backward_num_kernels(False) == 1 + 12 * K
        assert plan.backward_num_kernels(True) == 34 * K - 4
        assert plan.backward_workspace_bytes(False) == 0
        assert plan.backward_workspace_bytes(True) == (2 + (K - 1 + 5) * planes) * H * W * 4
        # the forward's figures are what they were
        assert plan.num_kernels == 1 + 6 * K
        tiles = lambda n: (n + 63) // 64      # noqa: E731
        assert plan.workspace_bytes == 2 * H * W * 4 + max(tiles(W) * H, tiles(H) * W) * 7 * planes * 4


def test_smooth_timed_capacity_is_checked():
    with host_smooth(K=2) as plan:
        L = capi.lib()
        one = arr([A])
        for edges, need in ((0, 25), (1, 64)):
            status = L.rf_smooth_plan_backward_timed(plan._h, one, None, one, one, None, edges, None, (ctypes.c_float * 5)(), None, 5)
            assert status == capi.RF_ERR_INVALID_ARG and f"need {need}".encode() in L.rf_last_error_string()
