"""GPU tests of the differentiable smoothing plan: rf_var_plan_backward_power (the ADJ && POWER instances and the POWER instances
of var_grad in kernels_var.hip), rf_var_distances_backward (var_distances_grad) and rf_smooth_plan_backward (plan_smooth.cpp),
through VarPlan.backward_power / apply_power, domain_transform_distances_backward, SmoothPlan.backward / apply and
edge_aware_smooth(form="plan", differentiable=True) of recfilter_amd/varscan.py, and the C++ front-end.

Reference: the f64 loops of tests/smooth_grad_loops.py (pinned against central differences and torch's autograd by
tests/test_smooth_grad_host.py).  Bar, per gradient (image, each exponent plane, guide) separately: max abs error over that
gradient's f64 peak <= max(4 x the same figure of the f32 serial loops, 1e-6); no NaN.  Cases: tests/smooth_grad_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guarded
import smooth_grad_cases as cases
import smooth_grad_loops as sloops
import var_grad_cases as vcases
import recfilter_amd as rfa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_LISTS = vcases.SCAN_LISTS
ALL = SCAN_LISTS["+x-x+y-y"]
BASES = cases.POWER_BASES
EXACT = (1, 70, 260)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def devs(arrays):
    return [dev(a) for a in arrays]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def nan_planes(shape_hw, n):
    import torch
    return [torch.full(shape_hw, np.nan, device="cuda") for _ in range(n)]


def run_power(shape, scans, ins, ds, bases, g, with_exponents, inplace=False):
    """one backward_power call on a fresh plan: (grad_ins, grad_exponents or None) on the host"""
    import torch
    hw = tuple(shape[1:])
    with rfa.VarPlan(hw, scans, planes=shape[0], n_weights=2) as plan:
        d_g = devs(g)
        read = {k for _, _, k in scans}
        d_gd = [nan_planes(hw, 1)[0] if k in read else None for k in range(2)] if with_exponents else None
        gin, gd = plan.backward_power(devs(ins) if with_exponents else None, devs(ds), bases, d_g, d_g if inplace else None, d_gd)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in gin], None if gd is None else [None if t is None else t.cpu().numpy() for t in gd]


# ---- the power form's adjoint ---------------------------------------------------------------------------------------------------
POWER_CASES = [(s, n) for s in [(1, 70, 260), (3, 130, 132)] for n in SCAN_LISTS] + \
              [(s, "+x-x+y-y") for s in cases.SHAPES if s not in [(1, 70, 260), (3, 130, 132)]]


@pytest.mark.parametrize("shape,name", POWER_CASES)
def test_backward_power_against_f64_loops(shape, name):
    """exponent planes with NaN at element 0: it reaches nothing"""
    ins, ds, g = list(cases.image(shape)), cases.exponent_planes(shape), list(cases.grad_out(shape))
    want_in, want_d, err_in, err_d = cases.expected_power(shape, name)
    image_only, none = run_power(shape, SCAN_LISTS[name], ins, ds, BASES, g, False)
    assert none is None
    gin, gd = run_power(shape, SCAN_LISTS[name], ins, ds, BASES, g, True)
    what = f"{shape} {name} power"
    cases.assert_under_bar(gin, want_in, err_in, f"{what} grad_in")
    for k in range(2):
        if want_d[k] is None:
            assert gd[k] is None
            continue
        cases.assert_under_bar([gd[k]], [want_d[k]], err_d[k], f"{what} grad_d[{k}]")
        first = gd[k][:, 0] if k == 0 else gd[k][0, :]
        assert np.array_equal(bits(first), np.zeros_like(bits(first))), f"{what} grad_d[{k}]: element 0 is not exactly 0"
    for a, b in zip(image_only, gin):      # the image gradient does not depend on whether exponent gradients were asked for
        np.testing.assert_array_equal(bits(a), bits(b))


def test_exponents_of_infinity_pass_the_gradient_through():
    ins, g = list(cases.image(EXACT)), list(cases.grad_out(EXACT))
    ds = [np.full(EXACT[1:], np.inf, dtype=np.float32) for _ in range(2)]
    gin, gd = run_power(EXACT, ALL, ins, ds, BASES, g, True)
    np.testing.assert_array_equal(bits(gin[0]), bits(g[0]))
    for k in range(2):
        np.testing.assert_array_equal(bits(gd[k]), np.zeros_like(bits(gd[k])))


def test_exponents_of_zero_give_the_plane_forms_gradient_at_one():
    ins, g = list(cases.image(EXACT)), list(cases.grad_out(EXACT))
    ds = [np.zeros(EXACT[1:], dtype=np.float32) for _ in range(2)]
    ones = [np.ones(EXACT[1:]) for _ in range(2)]
    _, plane_w = sloops.loops.backward(ins, ones, ALL, g, np.float64)
    _, ser_d = sloops.power_backward(ins, ds, BASES, ALL, g, np.float32)
    gin, gd = run_power(EXACT, ALL, ins, ds, BASES, g, True)
    assert not np.isnan(gin[0]).any()
    for k in range(2):
        want = sloops.constants(BASES[k], np.float64)[1] * plane_w[k]
        cases.assert_under_bar([gd[k]], [want], cases.figures([ser_d[k]], [want])[0], f"d = 0, grad_d[{k}]")


@pytest.mark.parametrize("shape", [(1, 70, 260), (3, 130, 132)])
def test_power_form_against_plane_form(shape):
    """`backward` on the weights exp2(d * l_k) formed on the host by the forward's convention (numpy's exp2 where the kernels use
    the hardware's: not bitwise) and `backward_power` on d: both image gradients under the power form's bar against one truth"""
    import torch
    ins, ds, g = list(cases.image(shape)), cases.exponent_planes(shape), list(cases.grad_out(shape))
    want_in, _, err_in, _ = cases.expected_power(shape, "+x-x+y-y")
    ws = [sloops.power_weights(np.nan_to_num(d, nan=1.0), a, np.float32) for d, a in zip(ds, BASES)]
    with rfa.VarPlan(shape[1:], ALL, planes=shape[0], n_weights=2) as plan:
        by_planes, _ = plan.backward(None, devs(ws), devs(g))
        by_power, _ = plan.backward_power(None, devs(ds), BASES, devs(g))
        torch.cuda.synchronize()
    cases.assert_under_bar([t.cpu().numpy() for t in by_planes], want_in, err_in, f"{shape} plane form on exp2(d l)")
    cases.assert_under_bar([t.cpu().numpy() for t in by_power], want_in, err_in, f"{shape} power form")


# ---- the distances' adjoint -----------------------------------------------------------------------------------------------------
def distance_gradients(shape_hw):
    rng = np.random.default_rng(2019)
    return [(rng.random(shape_hw) * 2 - 1).astype(np.float32) for _ in range(2)]


@pytest.mark.parametrize("shape", cases.SHAPES)
@pytest.mark.parametrize("channels", [1, 3])
def test_distances_backward_against_f64_loops(shape, channels):
    import torch
    hw = tuple(shape[1:])
    guide = cases.guide(shape, channels)
    gdx, gdy = distance_gradients(hw)
    want = sloops.distances_backward(guide, cases.SCALE, gdx, gdy, np.float64)
    serial = sloops.distances_backward(guide, cases.SCALE, gdx, gdy, np.float32)
    d_guide, d_gdx, d_gdy = dev(guide), dev(gdx), dev(gdy)
    run = lambda **kw: rfa.domain_transform_distances_backward(d_guide, cases.SIGMA_S, cases.SIGMA_R, d_gdx, d_gdy, **kw)      # noqa: E731
    got = run(grad_guide=torch.full((channels,) + hw, np.nan, device="cuda"))
    again = run()
    pattern = (np.random.default_rng(2020).random(guide.shape) * 2 - 1).astype(np.float32)
    added = run(grad_guide=dev(pattern), accumulate=True)
    torch.cuda.synchronize()
    what = f"distances backward {shape} x {channels}"
    cases.assert_under_bar([got.cpu().numpy()], [want], cases.figures([serial], [want])[0], what)
    guarded.assert_bits_equal([again.cpu()], [got.cpu()], f"{what}: two runs")
    cases.assert_under_bar([added.cpu().numpy()], [pattern.astype(np.float64) + want], cases.figures([pattern + serial], [pattern + want])[0],
                           f"{what}, accumulate")


def test_distances_backward_of_a_constant_guide_is_exactly_zero():
    import torch
    shape = (3, 130, 132)
    gdx, gdy = distance_gradients(shape[1:])
    got = rfa.domain_transform_distances_backward(torch.full(shape, 0.375, device="cuda"), cases.SIGMA_S, cases.SIGMA_R, dev(gdx), dev(gdy))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(got.cpu().numpy()), np.zeros(shape, dtype=np.uint32))


# ---- the plan's adjoint ---------------------------------------------------------------------------------------------------------
def smooth_plan(shape, K, self_guided, **kw):
    return rfa.SmoothPlan(shape[1:], planes=shape[0], guide_planes=0 if self_guided else shape[0], iterations=K, sigma_s=cases.SIGMA_S,
                          sigma_r=cases.SIGMA_R, **kw)


def expected_names(K, edges):
    fwd = ["var_tails_x", "var_carry", "var_pass2_x", "var_tails_y", "var_carry", "var_pass2_y"]
    adj = []
    for axis in "yyxx":
        adj += [f"var_adj_tails_{axis}", "var_carry", f"var_adj_pass2_{axis}"] + ([f"var_grad_{axis}"] if edges else [])
    fwd_scans = []
    for axis in "xxyy":
        fwd_scans += [f"var_tails_{axis}", "var_carry", f"var_pass2_{axis}"]
    if not edges:
        return ["var_distances"] + adj * K
    return ["var_distances"] + fwd * (K - 1) + (fwd_scans + adj) * K + ["var_distances_grad"]


@pytest.mark.parametrize("shape,K", cases.CASES)
@pytest.mark.parametrize("self_guided", [False, True])
def test_smooth_backward(shape, K, self_guided):
    """both settings of edges under the bar, and the bit-for-bit claims: against K backward_power calls, edges 0 against 1, repeated
    calls, in place against out of place; the launch names of the timed form"""
    import torch
    image, g = dev(cases.image(shape)), dev(cases.grad_out(shape))
    guide = None if self_guided else dev(cases.guide(shape))
    what = f"{shape} K={K} {'self' if self_guided else 'guide'}"
    with smooth_plan(shape, K, self_guided) as plan:
        held_im, none = plan.backward(image if self_guided else None, guide, g, edges=False)
        assert none is None
        full_im, full_gd = plan.backward(image, guide, g, None, None if self_guided else torch.full_like(guide, np.nan), edges=True)
        again_im, again_gd = plan.backward(image, guide, g, edges=True)
        in_place = g.clone()
        plan.backward(image, guide, in_place, in_place, edges=True)
        timed = [plan.backward_timed(image, guide, g, edges=e) for e in (False, True)]
        bases = plan.bases
        torch.cuda.synchronize()
    for edges in (False, True):
        want_im, want_gd, err_im, err_gd = cases.expected(shape, K, self_guided, edges)
        got = held_im if not edges else full_im
        cases.assert_under_bar([got.cpu().numpy()], [want_im], err_im, f"{what} edges={int(edges)} image")
        if edges and not self_guided:
            cases.assert_under_bar([full_gd.cpu().numpy()], [want_gd], err_gd, f"{what} guide")
        names = [n for n, _ in timed[int(edges)][2]]
        assert names == expected_names(K, edges), names
        guarded.assert_bits_equal([timed[int(edges)][0].cpu()], [got.cpu()], f"{what}: the timed form")
    guarded.assert_bits_equal([again_im.cpu()], [full_im.cpu()], f"{what}: two runs, image")
    guarded.assert_bits_equal([in_place.cpu()], [full_im.cpu()], f"{what}: in place")
    if not self_guided:
        guarded.assert_bits_equal([again_gd.cpu()], [full_gd.cpu()], f"{what}: two runs, guide")
        guarded.assert_bits_equal([full_im.cpu()], [held_im.cpu()], f"{what}: the image gradient with and without edges")
    # K calls of backward_power in reverse order on the library's own distance planes
    ds = list(rfa.domain_transform_distances(image if self_guided else guide, cases.SIGMA_S, cases.SIGMA_R))
    with rfa.VarPlan(shape[1:], ALL, planes=shape[0], n_weights=2) as var:
        grads = [g[c] for c in range(shape[0])]
        for k in range(K - 1, -1, -1):
            grads, _ = var.backward_power(None, ds, [bases[k], bases[k]], grads)
        torch.cuda.synchronize()
    guarded.assert_bits_equal([torch.stack(grads).cpu()], [held_im.cpu()], f"{what}: edges=0 against K backward_power calls")


@pytest.mark.parametrize("shape", [(1, 70, 260), (3, 130, 132)])
@pytest.mark.parametrize("self_guided", [False, True])
def test_guarded_planes_smooth_backward(shape, self_guided):
    """nothing is written outside grad_image / grad_guide; image, guide and grad_out are unchanged (their guards hold NaN)"""
    import torch
    C, hw, K = shape[0], tuple(shape[1:]), 2
    ims, g_im = guarded.guarded_planes(hw, np.float32, C, fill=guarded.IN_FILL)
    gos, g_go = guarded.guarded_planes(hw, np.float32, C, fill=guarded.IN_FILL)
    gds, g_gd = guarded.guarded_planes(hw, np.float32, C, fill=guarded.IN_FILL)
    g_im.load(devs(cases.image(shape)))
    g_go.load(devs(cases.grad_out(shape)))
    g_gd.load(devs(cases.guide(shape)))
    for checker in (g_im, g_go, g_gd):
        checker.snapshot()
    with smooth_plan(shape, K, self_guided) as plan:
        for edges in (False, True):
            outs, g_out = guarded.guarded_planes(hw, np.float32, C)
            ggs, g_gg = guarded.guarded_planes(hw, np.float32, C)
            plan.backward(ims, None if self_guided else gds, gos, outs, ggs if edges and not self_guided else None, edges=edges)
            torch.cuda.synchronize()
            g_out.check_guards("grad_image")
            g_gg.check_guards("grad_guide")
            for checker, name in ((g_im, "image"), (g_go, "grad_out"), (g_gd, "guide")):
                checker.check_unchanged(name)
            want_im, want_gd, err_im, err_gd = cases.expected(shape, K, self_guided, edges)
            cases.assert_under_bar([torch.stack(outs).cpu().numpy()], [want_im], err_im, f"guarded {shape} edges={int(edges)} image")
            if edges and not self_guided:
                cases.assert_under_bar([torch.stack(ggs).cpu().numpy()], [want_gd], err_gd, f"guarded {shape} guide")


def test_a_smooth_plan_keeps_no_state():
    import torch
    shape, K = (1, 70, 260), 2
    image, guide, g = dev(cases.image(shape)), dev(cases.guide(shape)), dev(cases.grad_out(shape))
    other = torch.full(shape, np.nan, device="cuda")
    with smooth_plan(shape, K, False) as plan:
        before = plan.execute(image, guide)
        results = []
        for step in range(3):
            gi, gg = plan.backward(image, guide, g, edges=True)
            results.append([gi.cpu(), gg.cpu()])
            plan.execute(other, guide)                             # an execute and a backward on other inputs in between
            plan.backward(other, other, other, edges=bool(step % 2))
        after = plan.execute(image, guide)
        torch.cuda.synchronize()
    for r in results[1:]:
        guarded.assert_bits_equal(r, results[0], "repeated backward calls of one smoothing plan")
    guarded.assert_bits_equal([after.cpu()], [before.cpu()], "execute before and after backward calls")
    with smooth_plan(shape, K, False) as fresh:
        gi, gg = fresh.backward(image, guide, g, edges=True)
        torch.cuda.synchronize()
    guarded.assert_bits_equal(results[0], [gi.cpu(), gg.cpu()], "against a fresh plan")


def test_smooth_backward_refusals_on_a_device_plan():
    """what a host-only plan cannot reach: alignment and overlap, decided before any launch (nothing is written)"""
    import torch
    shape, K = (1, 40, 64), 2
    image, guide, g = dev(cases.image(shape)), dev(cases.guide(shape)), dev(cases.grad_out(shape))
    with smooth_plan(shape, K, False) as plan:
        untouched = torch.full((1, 40, 68), 7.0, device="cuda")
        for args, text in (((image, guide, g, image), "grad_image plane 0 overlaps image plane 0"),
                           ((image, guide, g, guide), "grad_image plane 0 overlaps guide plane 0"),
                           ((image, guide, g, None, g), "gradient of guide plane 0 overlaps grad_out plane 0"),
                           ((image, guide, g, None, image), "gradient of guide plane 0 overlaps image plane 0")):
            with pytest.raises(rfa.RecFilterError, match=text) as e:
                plan.backward(*args, edges=True)
            assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG
        both = torch.empty((2, 40, 64), device="cuda")
        with pytest.raises(rfa.RecFilterError, match="grad_image plane 0 overlaps gradient of guide plane 0"):
            plan.backward(image, guide, g, both[0:1], both[0:1], edges=True)
        misaligned = untouched.reshape(-1)[1:1 + 40 * 64].view(1, 40, 64)
        with pytest.raises(rfa.RecFilterError, match="16-byte aligned"):
            plan.backward(image, guide, g, misaligned, edges=True)
        torch.cuda.synchronize()
        assert bool((untouched == 7.0).all())
    with smooth_plan(shape, K, False, guide_dtype=torch.uint8) as plan:
        g8 = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        with pytest.raises(rfa.RecFilterError) as e:
            plan.backward(image, g8, g, edges=True)
        assert e.value.status == rfa.capi.RF_ERR_UNSUPPORTED
        gi, _ = plan.backward(None, g8, g, edges=False)      # a byte guide is allowed with the distances held constant
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(gi.cpu().numpy()), bits(smooth_plan_constant_guide(shape, K, g)))


def smooth_plan_constant_guide(shape, K, g):
    """the image gradient with an f32 guide of zeros: a byte guide of zeros gives the same distances (all 1)"""
    import torch
    with smooth_plan(shape, K, False) as plan:
        gi, _ = plan.backward(None, torch.zeros(shape, device="cuda"), g, edges=False)
        torch.cuda.synchronize()
        return gi.cpu().numpy()


# ---- autograd -------------------------------------------------------------------------------------------------------------------
def autograd_case():
    import torch
    C, H, W, K = 3, 24, 36, 2
    rng = np.random.default_rng(2021)
    image = torch.from_numpy((rng.random((C, H, W)) * 2 - 1).astype(np.float32))
    guide = torch.from_numpy((0.5 * rng.random((C, H, W)) + np.linspace(0, 1, W)).astype(np.float32))      # seeded, no ties
    assert (guide[:, :, 1:] != guide[:, :, :-1]).all() and (guide[:, 1:, :] != guide[:, :-1, :]).all()
    g_out = torch.from_numpy((rng.random((C, H, W)) * 2 - 1).astype(np.float32))
    return image, guide, g_out, K, 8.0, 0.6


@pytest.mark.parametrize("through", ["SmoothPlan.apply", "edge_aware_smooth"])
def test_autograd_through_the_plan(through):
    import torch
    image, guide, g_out, K, sigma_s, sigma_r = autograd_case()
    C, H, W = image.shape
    bases = [float(np.float32(a)) for a in rfa.domain_transform_bases(sigma_s, K)]

    def reference(dtype):
        im, gd = image.clone().to(dtype).requires_grad_(True), guide.clone().to(dtype).requires_grad_(True)
        sloops.torch_filter(im, gd, bases, float(np.float32(sigma_s / sigma_r)), dtype).backward(g_out.to(dtype))
        return im.grad.numpy(), gd.grad.numpy()
    want, serial = reference(torch.float64), reference(torch.float32)
    d_im, d_gd = image.cuda().requires_grad_(True), guide.cuda().requires_grad_(True)
    plan = rfa.SmoothPlan((H, W), planes=C, guide_planes=C, iterations=K, sigma_s=sigma_s, sigma_r=sigma_r)
    if through == "SmoothPlan.apply":
        smooth = lambda im, gd: plan.apply(im, gd)      # noqa: E731
    else:
        smooth = lambda im, gd: rfa.edge_aware_smooth(im, guide=gd, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, form="plan",      # noqa: E731
                                                      differentiable=True)
    out = smooth(d_im, d_gd)
    assert out.grad_fn is not None
    out.backward(g_out.cuda())
    torch.cuda.synchronize()
    for what, got, w, s in (("image", d_im.grad, want[0], serial[0]), ("guide", d_gd.grad, want[1], serial[1])):
        cases.assert_under_bar([got.cpu().numpy()], [w], cases.figures([s], [w])[0], f"{through} gradient, {what}")
    # the forward values are those of form="plan" without the flag, and under no_grad nothing is recorded
    plain = rfa.edge_aware_smooth(image.cuda(), guide=guide.cuda(), sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, form="plan")
    assert plain.grad_fn is None
    with torch.no_grad():
        muted = smooth(d_im, d_gd)
    assert muted.grad_fn is None
    torch.cuda.synchronize()
    guarded.assert_bits_equal([out.detach().cpu(), muted.cpu()], [plain.cpu(), plain.cpu()], f"{through}: forward values")
    # only the image requires a gradient: the distances are held constant, and the image gradient is the same bits
    only_im = image.cuda().requires_grad_(True)
    smooth(only_im, guide.cuda()).backward(g_out.cuda())
    torch.cuda.synchronize()
    guarded.assert_bits_equal([only_im.grad.cpu()], [d_im.grad.cpu()], f"{through}: image gradient without a guide gradient")
    # an image that guides itself
    self_guided = image.cuda().requires_grad_(True)
    if through == "SmoothPlan.apply":
        with rfa.SmoothPlan((H, W), planes=C, iterations=K, sigma_s=sigma_s, sigma_r=sigma_r) as self_plan:
            self_plan.apply(self_guided).backward(g_out.cuda())
            torch.cuda.synchronize()
    else:
        rfa.edge_aware_smooth(self_guided, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, form="plan", differentiable=True).backward(g_out.cuda())
        torch.cuda.synchronize()
    assert self_guided.grad is not None and not torch.isnan(self_guided.grad).any()
    im64 = image.clone().double().requires_grad_(True)
    sloops.torch_filter(im64, None, bases, float(np.float32(sigma_s / sigma_r)), torch.float64).backward(g_out.double())
    im32 = image.clone().requires_grad_(True)
    sloops.torch_filter(im32, None, bases, float(np.float32(sigma_s / sigma_r)), torch.float32).backward(g_out)
    cases.assert_under_bar([self_guided.grad.cpu().numpy()], [im64.grad.numpy()], cases.figures([im32.grad.numpy()], [im64.grad.numpy()])[0],
                           f"{through} gradient, self-guided image")
    plan.close()


def test_differentiable_flag_and_forms():
    import torch
    image, guide, _, K, sigma_s, sigma_r = autograd_case()
    d_im = image.cuda().requires_grad_(True)
    with pytest.raises(ValueError, match="plan"):
        rfa.edge_aware_smooth(d_im, guide=guide.cuda(), iterations=K, form="power", differentiable=True)
    # the default stays off, and the flag changes nothing for form="planes"
    assert rfa.edge_aware_smooth(d_im, guide=guide.cuda(), sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, form="plan").grad_fn is None
    a = rfa.edge_aware_smooth(d_im, guide=guide.cuda(), sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, form="planes", differentiable=True)
    b = rfa.edge_aware_smooth(d_im, guide=guide.cuda(), sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, form="planes")
    torch.cuda.synchronize()
    assert a.grad_fn is not None and b.grad_fn is not None
    guarded.assert_bits_equal([a.detach().cpu()], [b.detach().cpu()], 'form="planes" with and without the flag')


def test_apply_power():
    import torch
    shape = (3, 130, 132)
    ins, ds, g = list(cases.image(shape)), cases.exponent_planes(shape), list(cases.grad_out(shape))
    want_in, want_d, err_in, err_d = cases.expected_power(shape, "+x-x+y-y")
    with rfa.VarPlan(shape[1:], ALL, planes=3, n_weights=2) as plan:
        d_ins = [t.requires_grad_(True) for t in devs(ins)]
        d_ds = devs(ds)
        d_ds[1].requires_grad_(True)      # needs_input_grad decides: only the y plane gets a gradient
        outs = plan.apply_power(d_ins, d_ds, BASES)
        direct = plan.execute_power(devs(ins), devs(ds), BASES)
        torch.autograd.backward(list(outs), devs(g))
        torch.cuda.synchronize()
        guarded.assert_bits_equal([t.detach().cpu() for t in outs], [t.cpu() for t in direct], "apply_power against execute_power")
        assert d_ds[0].grad is None
        cases.assert_under_bar([t.grad.cpu().numpy() for t in d_ins], want_in, err_in, "apply_power grad_in")
        cases.assert_under_bar([d_ds[1].grad.cpu().numpy()], [want_d[1]], err_d[1], "apply_power grad_d[1]")
        with torch.no_grad():
            assert plan.apply_power(d_ins, d_ds, BASES)[0].grad_fn is None


# ---- the C++ front-end ----------------------------------------------------------------------------------------------------------
def test_cpp_frontend_smooth_grad(tmp_path):
    """RecFilterSmooth::gradient and RecFilterVarying::gradient_power on 70 x 260 against loops in the C++ file, under the bar
    above; compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_smooth_grad.cpp")
    exe = str(tmp_path / "test_frontend_smooth_grad")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "smooth-grad-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
