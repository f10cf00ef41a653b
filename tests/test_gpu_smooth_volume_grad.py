"""GPU tests of the differentiable smoothing plan on volumes: rf_var_distances_volume_backward (var_distances_volume_grad in
kernels_var.hip) and rf_smooth_plan_backward on plans created with RF_SMOOTH_VOLUME_BACKWARD (plan_smooth.cpp), through
domain_transform_distances_volume_backward, SmoothPlan.volume(..., differentiable=True).backward / backward_timed / apply and
edge_aware_smooth_volume(..., differentiable=True) of recfilter_amd/varscan.py, and the C++ front-end.

Reference: the f64 loops of tests/smooth_volume_grad_loops.py (pinned against central differences and torch's autograd by
tests/test_smooth_volume_grad_host.py).  Bar, per gradient separately: max abs error over that gradient's f64 peak
<= max(4 x the same figure of the f32 serial loops, 1e-6); no NaN.  Cases: tests/smooth_volume_grad_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guarded
import recfilter_amd as rfa
import smooth_volume_grad_cases as cases
import smooth_volume_grad_loops as vsloops
from recfilter_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, R, SPACING = cases.SIGMA_S, cases.SIGMA_R, cases.SPACING_Z


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the distances' adjoint -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.DISTANCE_SHAPES, ids=str)
def test_distances_backward_against_f64_loops(shape):
    """stored and accumulated under the bar; two runs bit for bit; NaN on the three faces reaches nothing; with gdz = 0 every slice
    holds the values of the image entry point"""
    import torch
    C, D, H, W = shape
    guide = cases.guide(shape)
    gds = cases.distance_gradients(shape)
    want, err32, want_sum, err32_sum = cases.expected_distances(shape)
    d_guide, d_gds = dev(guide), [dev(a) for a in gds]
    run = lambda g=d_gds, **kw: rfa.domain_transform_distances_volume_backward(d_guide, S, R, g[0], g[1], g[2], **kw)      # noqa: E731
    got = run(grad_guide=torch.full(shape, np.nan, device="cuda"))
    again = run()
    added = run(grad_guide=dev(cases.accumulate_pattern(shape)), accumulate=True)
    poisoned = [t.clone() for t in d_gds]
    poisoned[0][:, :, 0], poisoned[1][:, 0, :], poisoned[2][0] = np.nan, np.nan, np.nan
    faces = run(poisoned)
    flat = run([d_gds[0], d_gds[1], torch.zeros_like(d_gds[2])])
    torch.cuda.synchronize()
    what = f"volume distances backward {shape}"
    assert tuple(got.shape) == shape
    cases.assert_under_bar([got.cpu().numpy()], [want], err32, what)
    cases.assert_under_bar([added.cpu().numpy()], [want_sum], err32_sum, f"{what}, accumulate")
    guarded.assert_bits_equal([again.cpu()], [got.cpu()], f"{what}: two runs")
    guarded.assert_bits_equal([faces.cpu()], [got.cpu()], f"{what}: NaN in gdx[:, :, 0], gdy[:, 0, :] and gdz[0]")
    for z in range(D):
        slice_ = rfa.domain_transform_distances_backward(d_guide[:, z].contiguous(), S, R, d_gds[0][z].contiguous(), d_gds[1][z].contiguous())
        assert np.array_equal(flat[:, z].cpu().numpy(), slice_.cpu().numpy()), f"{what}: slice {z} with gdz = 0 against the image entry point"


def test_distances_backward_of_a_constant_guide_is_exactly_zero():
    import torch
    shape = (3, 20, 66, 68)
    gds = [dev(a) for a in cases.distance_gradients(shape)]
    got = rfa.domain_transform_distances_volume_backward(torch.full(shape, 0.375, device="cuda"), S, R, *gds)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), np.zeros(shape, dtype=np.float32))


def test_distances_backward_of_a_single_volume_and_guards():
    """a (D, H, W) guide; nothing is written outside the gradient volume, and the inputs (their guards hold NaN) are unchanged"""
    import torch
    shape = cases.SHAPES[0]
    dhw = shape[1:]
    d_g, c_g = guarded.guarded_planes(dhw, np.float32, 1, fill=guarded.IN_FILL)
    d_gd, c_gd = guarded.guarded_planes(dhw, np.float32, 3, fill=guarded.IN_FILL)
    d_out, c_out = guarded.guarded_planes(dhw, np.float32, 1, fill=guarded.OUT_FILL)
    c_g.load([dev(cases.guide(shape)[0])])
    c_gd.load([dev(a) for a in cases.distance_gradients(shape)])
    c_g.snapshot()
    c_gd.snapshot()
    got = rfa.domain_transform_distances_volume_backward(d_g[0], S, R, d_gd[0], d_gd[1], d_gd[2], grad_guide=d_out[0])
    torch.cuda.synchronize()
    assert tuple(got.shape) == dhw
    c_out.check_guards("gradient of the guide")
    c_g.check_unchanged("guide")
    c_gd.check_unchanged("distance gradients")
    want = rfa.domain_transform_distances_volume_backward(dev(cases.guide(shape)[:1]), S, R, *[dev(a) for a in cases.distance_gradients(shape)])
    guarded.assert_bits_equal([got.cpu()], [want[0].cpu()], "guarded volumes against plain ones")


# ---- the plan's adjoint ---------------------------------------------------------------------------------------------------------
def smooth_plan(shape, K, guide_kind, differentiable=True):
    import torch
    n_guide = {"self": 0, "f32": shape[0], "u8": cases.BYTE_GUIDE_CHANNELS}[guide_kind]
    return rfa.SmoothPlan.volume(shape[1:], planes=shape[0], guide_planes=n_guide, guide_dtype=torch.uint8 if guide_kind == "u8" else None,
                                 iterations=K, sigma_s=S, sigma_r=R, spacing_z=SPACING, differentiable=differentiable)


@pytest.mark.parametrize("shape,K", cases.CASES, ids=str)
@pytest.mark.parametrize("self_guided", [False, True])
def test_smooth_backward(shape, K, self_guided):
    """both settings of edges under the bar, and the bit-for-bit claims: against K backward_power calls, edges 0 against 1, repeated
    calls, in place against out of place; the launch names of the timed form"""
    import torch
    kind = "self" if self_guided else "f32"
    image, g = dev(cases.image(shape)), dev(cases.grad_out(shape))
    guide = None if self_guided else dev(cases.guide(shape))
    what = f"volume {shape} K={K} {kind}"
    with smooth_plan(shape, K, kind) as plan:
        assert plan.backward_num_kernels(False) == 1 + 18 * K and plan.backward_num_kernels(True) == 51 * K - 7
        held_im, none = plan.backward(image if self_guided else None, guide, g, edges=False)
        assert none is None
        full_im, full_gd = plan.backward(image, guide, g, None, None if self_guided else torch.full_like(guide, np.nan), edges=True)
        again_im, again_gd = plan.backward(image, guide, g, edges=True)
        in_place = g.clone()
        plan.backward(image, guide, in_place, in_place, edges=True)
        held_in_place = g.clone()
        plan.backward(image if self_guided else None, guide, held_in_place, held_in_place, edges=False)
        timed = [plan.backward_timed(image, guide, g, edges=e) for e in (False, True)]
        bases = plan.bases
        torch.cuda.synchronize()
    for edges in (False, True):
        want_im, want_gd, err_im, err_gd = cases.expected(shape, K, kind, edges)
        got = held_im if not edges else full_im
        cases.assert_under_bar([got.cpu().numpy()], [want_im], err_im, f"{what} edges={int(edges)} image")
        if edges and not self_guided:
            cases.assert_under_bar([full_gd.cpu().numpy()], [want_gd], err_gd, f"{what} guide")
        names = [n for n, _ in timed[int(edges)][2]]
        assert names == cases.expected_names(K, edges), names
        guarded.assert_bits_equal([timed[int(edges)][0].cpu()], [got.cpu()], f"{what}: the timed form")
    guarded.assert_bits_equal([again_im.cpu()], [full_im.cpu()], f"{what}: two runs, image")
    guarded.assert_bits_equal([in_place.cpu()], [full_im.cpu()], f"{what}: in place, edges = 1")
    guarded.assert_bits_equal([held_in_place.cpu()], [held_im.cpu()], f"{what}: in place, edges = 0")
    if not self_guided:
        guarded.assert_bits_equal([again_gd.cpu()], [full_gd.cpu()], f"{what}: two runs, guide")
        guarded.assert_bits_equal([full_im.cpu()], [held_im.cpu()], f"{what}: the image gradient with and without edges")
    # K calls of backward_power in reverse order on the library's own distance volumes
    ds = list(rfa.domain_transform_distances_volume(image if self_guided else guide, S, R, spacing_z=SPACING))
    with rfa.VarPlan.volume(shape[1:], vsloops.SCANS, planes=shape[0], n_weights=3) as var:
        grads = [g[c] for c in range(shape[0])]
        for k in range(K - 1, -1, -1):
            grads, _ = var.backward_power(None, ds, [bases[k]] * 3, grads)
        torch.cuda.synchronize()
    guarded.assert_bits_equal([torch.stack(grads).cpu()], [held_im.cpu()], f"{what}: edges=0 against K backward_power calls")


@pytest.mark.parametrize("shape,K", [cases.CASES[0], cases.CASES[3]], ids=str)
def test_a_byte_guide_with_the_distances_held_constant(shape, K):
    import torch
    g = dev(cases.grad_out(shape))
    guide = dev(cases.byte_guide(shape))
    with smooth_plan(shape, K, "u8") as plan:
        got, none = plan.backward(None, guide, g, edges=False)
        with pytest.raises(rfa.RecFilterError) as e:
            plan.backward(dev(cases.image(shape)), guide, g, edges=True)
        torch.cuda.synchronize()
    assert none is None and e.value.status == capi.RF_ERR_UNSUPPORTED
    want_im, _, err_im, _ = cases.expected(shape, K, "u8", False)
    cases.assert_under_bar([got.cpu().numpy()], [want_im], err_im, f"volume {shape} K={K} byte guide, edges=0 image")


@pytest.mark.parametrize("self_guided", [False, True])
def test_guarded_volumes_smooth_backward(self_guided):
    """one edges = 1 call: nothing is written outside grad_image / grad_guide; image, guide and grad_out are unchanged (their guards
    hold NaN)"""
    import torch
    shape, K = cases.CASES[0]
    kind = "self" if self_guided else "f32"
    C, dhw = shape[0], tuple(shape[1:])
    ims, g_im = guarded.guarded_planes(dhw, np.float32, C, fill=guarded.IN_FILL)
    gos, g_go = guarded.guarded_planes(dhw, np.float32, C, fill=guarded.IN_FILL)
    gds, g_gd = guarded.guarded_planes(dhw, np.float32, C, fill=guarded.IN_FILL)
    g_im.load(list(dev(cases.image(shape))))
    g_go.load(list(dev(cases.grad_out(shape))))
    g_gd.load(list(dev(cases.guide(shape))))
    for checker in (g_im, g_go, g_gd):
        checker.snapshot()
    outs, g_out = guarded.guarded_planes(dhw, np.float32, C)
    ggs, g_gg = guarded.guarded_planes(dhw, np.float32, C)
    with smooth_plan(shape, K, kind) as plan:
        plan.backward(ims, None if self_guided else gds, gos, outs, None if self_guided else ggs, edges=True)
        torch.cuda.synchronize()
    g_out.check_guards("grad_image")
    g_gg.check_guards("grad_guide")
    for checker, name in ((g_im, "image"), (g_go, "grad_out"), (g_gd, "guide")):
        checker.check_unchanged(name)
    want_im, want_gd, err_im, err_gd = cases.expected(shape, K, kind, True)
    cases.assert_under_bar([torch.stack(outs).cpu().numpy()], [want_im], err_im, f"guarded volume {shape} {kind} image")
    if not self_guided:
        cases.assert_under_bar([torch.stack(ggs).cpu().numpy()], [want_gd], err_gd, f"guarded volume {shape} guide")


def test_a_plan_keeps_no_state_and_the_forward_is_the_unflagged_plans():
    import torch
    shape, K = cases.CASES[1]
    image, guide, g = dev(cases.image(shape)), dev(cases.guide(shape)), dev(cases.grad_out(shape))
    other = torch.full(shape, np.nan, device="cuda")
    with smooth_plan(shape, K, "f32") as plan, smooth_plan(shape, K, "f32", differentiable=False) as plain:
        assert plan.num_kernels == plain.num_kernels and plan.workspace_bytes == plain.workspace_bytes
        before = plan.execute(image, guide)
        results = []
        for step in range(3):
            gi, gg = plan.backward(image, guide, g, edges=True)
            results.append([gi.cpu(), gg.cpu()])
            plan.execute(other, guide)                             # an execute and a backward on other inputs in between
            plan.backward(other, other, other, edges=bool(step % 2))
        after = plan.execute(image, guide)
        unflagged = plain.execute(image, guide)
        with pytest.raises(rfa.RecFilterError) as e:
            plain.backward(image, guide, g, edges=True)
        assert e.value.status == capi.RF_ERR_UNSUPPORTED
        torch.cuda.synchronize()
    for r in results[1:]:
        guarded.assert_bits_equal(r, results[0], "repeated backward calls of one volume plan")
    guarded.assert_bits_equal([after.cpu()], [before.cpu()], "execute before and after backward calls")
    guarded.assert_bits_equal([before.cpu()], [unflagged.cpu()], "a flagged plan's execute against an unflagged plan's")
    with smooth_plan(shape, K, "f32") as fresh:
        gi, gg = fresh.backward(image, guide, g, edges=True)
        torch.cuda.synchronize()
    guarded.assert_bits_equal(results[0], [gi.cpu(), gg.cpu()], "against a fresh plan")


def test_refusals_on_a_device_plan():
    """what a host-only plan cannot reach: alignment and overlap, decided before any launch"""
    import torch
    shape, K = cases.CASES[1]
    image, guide, g = dev(cases.image(shape)), dev(cases.guide(shape)), dev(cases.grad_out(shape))
    with smooth_plan(shape, K, "f32") as plan:
        for args, text in (((image, guide, g, image), "grad_image plane 0 overlaps image plane 0"),
                           ((image, guide, g, guide), "grad_image plane 0 overlaps guide plane 0"),
                           ((image, guide, g, None, g), "gradient of guide plane 0 overlaps grad_out plane 0")):
            with pytest.raises(rfa.RecFilterError, match=text) as e:
                plan.backward(*args, edges=True)
            assert e.value.status == capi.RF_ERR_INVALID_ARG
        spare = torch.zeros(int(np.prod(shape)) + 4, device="cuda")
        misaligned = spare[1:1 + int(np.prod(shape))].view(shape)
        with pytest.raises(rfa.RecFilterError, match="16-byte aligned"):
            plan.backward(image, guide, g, misaligned, edges=True)
        torch.cuda.synchronize()


# ---- autograd -------------------------------------------------------------------------------------------------------------------
def autograd_case():
    import torch
    C, D, H, W, K = 2, 6, 10, 12, 2
    rng = np.random.default_rng(2027)
    image = torch.from_numpy((rng.random((C, D, H, W)) * 2 - 1).astype(np.float32))
    guide = torch.from_numpy((0.5 * rng.random((C, D, H, W)) + np.linspace(0, 1, W) + np.linspace(0, 1, H)[:, None]
                              + np.linspace(0, 1, D)[:, None, None]).astype(np.float32))      # seeded, no ties
    assert (guide[..., 1:] != guide[..., :-1]).all() and (guide[:, :, 1:] != guide[:, :, :-1]).all() and (guide[:, 1:] != guide[:, :-1]).all()
    g_out = torch.from_numpy((rng.random((C, D, H, W)) * 2 - 1).astype(np.float32))
    return image, guide, g_out, K, 8.0, 0.6


@pytest.mark.parametrize("through", ["SmoothPlan.apply", "edge_aware_smooth_volume"])
def test_autograd_through_the_plan(through):
    import torch
    image, guide, g_out, K, sigma_s, sigma_r = autograd_case()
    C, D, H, W = image.shape
    bases = [float(np.float32(a)) for a in rfa.domain_transform_bases(sigma_s, K)]
    scale = float(np.float32(sigma_s / sigma_r))

    def reference(dtype, self_guided=False):
        im = image.clone().to(dtype).requires_grad_(True)
        gd = None if self_guided else guide.clone().to(dtype).requires_grad_(True)
        vsloops.torch_filter(im, gd, bases, scale, SPACING, dtype).backward(g_out.to(dtype))
        return im.grad.numpy(), None if self_guided else gd.grad.numpy()
    want, serial = reference(torch.float64), reference(torch.float32)
    d_im, d_gd = image.cuda().requires_grad_(True), guide.cuda().requires_grad_(True)
    plan = rfa.SmoothPlan.volume((D, H, W), planes=C, guide_planes=C, iterations=K, sigma_s=sigma_s, sigma_r=sigma_r, spacing_z=SPACING,
                                 differentiable=True)
    if through == "SmoothPlan.apply":
        smooth = lambda im, gd: plan.apply(im, gd)      # noqa: E731
    else:
        smooth = lambda im, gd: rfa.edge_aware_smooth_volume(im, gd, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, spacing_z=SPACING,      # noqa: E731
                                                             differentiable=True)
    out = smooth(d_im, d_gd)
    assert out.grad_fn is not None
    out.backward(g_out.cuda())
    torch.cuda.synchronize()
    for what, got, w, s in (("image", d_im.grad, want[0], serial[0]), ("guide", d_gd.grad, want[1], serial[1])):
        cases.assert_under_bar([got.cpu().numpy()], [w], cases.figures([s], [w])[0], f"{through} gradient, {what}")
    # the default call has no grad_fn and the same values; under no_grad nothing is recorded
    plain = rfa.edge_aware_smooth_volume(d_im, d_gd, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, spacing_z=SPACING)
    assert plain.grad_fn is None
    with torch.no_grad():
        muted = smooth(d_im, d_gd)
    assert muted.grad_fn is None
    torch.cuda.synchronize()
    guarded.assert_bits_equal([out.detach().cpu(), muted.cpu()], [plain.cpu(), plain.cpu()], f"{through}: forward values")
    # only the volume requires a gradient: the distances are held constant, and the image gradient is the same bits
    only_im = image.cuda().requires_grad_(True)
    smooth(only_im, guide.cuda()).backward(g_out.cuda())
    torch.cuda.synchronize()
    guarded.assert_bits_equal([only_im.grad.cpu()], [d_im.grad.cpu()], f"{through}: image gradient without a guide gradient")
    # a volume that guides itself
    self_guided = image.cuda().requires_grad_(True)
    if through == "SmoothPlan.apply":
        with rfa.SmoothPlan.volume((D, H, W), planes=C, iterations=K, sigma_s=sigma_s, sigma_r=sigma_r, spacing_z=SPACING, differentiable=True) as self_plan:
            self_plan.apply(self_guided).backward(g_out.cuda())
            torch.cuda.synchronize()
    else:
        rfa.edge_aware_smooth_volume(self_guided, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, spacing_z=SPACING, differentiable=True).backward(g_out.cuda())
        torch.cuda.synchronize()
    want_self, serial_self = reference(torch.float64, True)[0], reference(torch.float32, True)[0]
    cases.assert_under_bar([self_guided.grad.cpu().numpy()], [want_self], cases.figures([serial_self], [want_self])[0],
                           f"{through} gradient, self-guided volume")
    plan.close()


def test_differentiable_flag_and_dtypes():
    import torch
    image, guide, _, K, sigma_s, sigma_r = autograd_case()
    d_im = image.cuda().requires_grad_(True)
    byte_guide = (guide * 60).to(torch.uint8).cuda()
    # a byte guide that needs no gradient is fine (the distances are held constant) ...
    out = rfa.edge_aware_smooth_volume(d_im, byte_guide, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, differentiable=True)
    assert out.grad_fn is not None
    # ... a byte volume is not: nothing of it can require a gradient, so the call is the plain one
    plain = rfa.edge_aware_smooth_volume((image.abs() * 200).to(torch.uint8).cuda(), sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, differentiable=True)
    assert plain.grad_fn is None and plain.dtype == torch.uint8
    # a 64-bit volume is filtered in f32, as without the flag, and the gradient comes back in its own type
    d64 = image.double().cuda().requires_grad_(True)
    rfa.edge_aware_smooth_volume(d64, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, differentiable=True).sum().backward()
    torch.cuda.synchronize()
    assert d64.grad is not None and d64.grad.dtype == torch.float64 and not torch.isnan(d64.grad).any()


# ---- the C++ front-end ----------------------------------------------------------------------------------------------------------
def test_cpp_frontend_smooth_volume_grad(tmp_path):
    """RecFilterSmooth::differentiable / gradient on a 24 x 22 x 70 volume and domain_transform_distances_volume_gradient against loops
    in the C++ file, under the bar above; compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_smooth_volume_grad.cpp")
    exe = str(tmp_path / "test_frontend_smooth_volume_grad")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "smooth-volume-grad-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
