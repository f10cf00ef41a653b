"""GPU tests of the varying scans' adjoint (rf_var_plan_backward: the ADJ instances and var_grad of kernels_var.hip, plan_var.cpp,
VarPlan.backward / VarPlan.apply / var_scan / edge_aware_smooth of recfilter_amd/varscan.py).

Reference: the f64 loops of tests/var_grad_loops.py (pinned against central differences by tests/test_var_grad_host.py).  Bar, for
the image gradient and each weight gradient separately: max abs error over that gradient's f64 peak <= max(4 x the same figure of
the f32 serial loops, 1e-6); no NaN anywhere; element 0 of a weight gradient exactly 0.  Inputs and weights are those of
tests/test_gpu_var_scans.py (NaN at element 0 of the weights, mean 0.8), grad_out is seeded and signed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guarded
import var_grad_cases as cases
import recfilter_amd as rfa
from test_gpu_var_scans import PX, PY, MY, constant_weights, to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_LISTS, SHAPES = cases.SCAN_LISTS, cases.SHAPES
ALL = SCAN_LISTS["+x-x+y-y"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(tensors):
    return [t.cpu().numpy() for t in tensors]


def run_backward(shape, planes, scans, ins, ws, g, with_weights, inplace=False, n_weights=2):
    """one backward call on a fresh plan: (grad_ins, grad_weights or None) on the host"""
    import torch
    with rfa.VarPlan(shape, scans, planes=planes, n_weights=n_weights) as plan:
        d_g = to_device(g)
        read = {k for _, _, k in scans}
        d_gw = [torch.full(shape, np.nan, device="cuda") if k in read else None for k in range(n_weights)] if with_weights else None
        gin, gw = plan.backward(to_device(ins) if with_weights else None, to_device(ws), d_g, d_g if inplace else None, d_gw)
        torch.cuda.synchronize()
        return host(gin), None if gw is None else [None if t is None else t.cpu().numpy() for t in gw]


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCAN_LISTS))
@pytest.mark.parametrize("shape,planes", SHAPES)
def test_against_f64_loops(shape, planes, name):
    ins, ws = cases.case(shape, planes)
    g = cases.grad_out(shape, planes)
    image_only, none = run_backward(shape, planes, SCAN_LISTS[name], ins, ws, g, False)
    assert none is None
    gin, gw = run_backward(shape, planes, SCAN_LISTS[name], ins, ws, g, True)
    cases.assert_gradients(gin, gw, shape, planes, name, f"{shape} x {planes} {name}")
    for a, b in zip(image_only, gin):      # the image gradient does not depend on whether weight gradients were asked for
        np.testing.assert_array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", ["+x-x", "+y-y", "+x-x+y-y"])
def test_weights_with_exact_zeros_and_ones(name):
    shape, planes = (70, 260), 1
    ins, ws = cases.case(shape, planes, "sprinkled")
    gin, gw = run_backward(shape, planes, SCAN_LISTS[name], ins, ws, cases.grad_out(shape, planes), True)
    cases.assert_gradients(gin, gw, shape, planes, name, f"sprinkled {name}", "sprinkled")


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
EXACT_SHAPE = (70, 260)      # 5 tiles along x, 2 along y, the last one partial each way


def test_weights_of_zero():
    ins, _ = cases.case(EXACT_SHAPE, 1)
    g = cases.grad_out(EXACT_SHAPE, 1)
    for name in ("+x", "-x", "+y", "-y", "+x-x+y-y"):
        gin, _ = run_backward(EXACT_SHAPE, 1, SCAN_LISTS[name], ins, constant_weights(0.0), g, True)
        np.testing.assert_array_equal(bits(gin[0]), bits(g[0]), err_msg=name)
    _, gw = run_backward(EXACT_SHAPE, 1, SCAN_LISTS["+x"], ins, constant_weights(0.0), g, True)
    x = ins[0]
    want = np.zeros(EXACT_SHAPE, dtype=np.float32)
    want[:, 1:] = g[0][:, 1:] * (x[:, :-1] - x[:, 1:])      # the scan's output is its input; lam is grad_out
    np.testing.assert_array_equal(bits(gw[0]), bits(want))


def test_weights_of_one():
    ins, _ = cases.case(EXACT_SHAPE, 1)
    g = cases.grad_out(EXACT_SHAPE, 1)
    gin, gw = run_backward(EXACT_SHAPE, 1, SCAN_LISTS["+x"], ins, constant_weights(1.0), g, True)
    assert not np.isnan(gin[0]).any() and not np.isnan(gw[0]).any()
    np.testing.assert_array_equal(gin[0][:, 1:], np.zeros_like(gin[0][:, 1:]))      # every output is sample 0: the others have no say
    want = g[0].astype(np.float64).sum(axis=1)                                      # ... and sample 0 collects every grad_out
    np.testing.assert_allclose(gin[0][:, 0], want, rtol=0, atol=1e-5 * np.abs(g[0]).sum(axis=1).max())


# ---- in place, state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,planes", [((70, 260), 1), ((130, 132), 3)])
@pytest.mark.parametrize("with_weights", [False, True])
def test_in_place_equals_out_of_place(shape, planes, with_weights):
    ins, ws = cases.case(shape, planes)
    g = cases.grad_out(shape, planes)
    a_in, a_w = run_backward(shape, planes, ALL, ins, ws, g, with_weights)
    b_in, b_w = run_backward(shape, planes, ALL, ins, ws, g, with_weights, inplace=True)
    for p, q in zip(a_in + (a_w or []), b_in + (b_w or [])):
        np.testing.assert_array_equal(bits(p), bits(q))


def test_a_plan_keeps_no_state():
    import torch
    shape, planes = (70, 260), 1
    ins, ws = cases.case(shape, planes)
    g = cases.grad_out(shape, planes)
    other = [np.full(shape, np.nan, dtype=np.float32)]
    with rfa.VarPlan(shape, ALL, planes=planes, n_weights=2) as plan:
        d_in, d_w, d_g = to_device(ins), to_device(ws), to_device(g)
        before = plan.execute(d_in, d_w)
        results = []
        for step in range(3):
            gw = [torch.full(shape, np.nan, device="cuda") for _ in range(2)]
            gin, gw = plan.backward(d_in, d_w, d_g, None, gw)
            results.append([t.cpu() for t in gin + gw])
            plan.execute(to_device(other), d_w)                      # a forward execute and a different input in between
            plan.backward(to_device(other), d_w, to_device(other), None, [torch.empty(shape, device="cuda") for _ in range(2)])
        after = plan.execute(d_in, d_w)
        torch.cuda.synchronize()
        for r in results[1:]:
            guarded.assert_bits_equal(r, results[0], "repeated backward calls of one plan")
        guarded.assert_bits_equal([t.cpu() for t in after], [t.cpu() for t in before], "execute before and after backward calls")
    fresh_in, fresh_w = run_backward(shape, planes, ALL, ins, ws, g, True)
    guarded.assert_bits_equal(results[0], [torch.from_numpy(a) for a in fresh_in + fresh_w], "against a fresh plan")


# ---- which planes get a gradient --------------------------------------------------------------------------------------------------
def test_a_plane_read_along_both_dimensions_gets_the_sum():
    import var_grad_loops as loops
    shape = (70, 260)
    ins, ws = cases.case(shape, 1)
    g = cases.grad_out(shape, 1)
    w = np.array(ws[0])
    w[:, 0] = ws[1][:, 0]                              # column 0 is read by the y scan, row 0 by the x scans:
    w[0, 0] = np.nan                                   # the one element neither reads
    scans = [(0, True, 0), (1, False, 0), (0, False, 0)]
    gin, gw = run_backward(shape, 1, scans, ins, [w], g, True, n_weights=1)
    want_in, want_w = loops.backward(ins, [w], scans, g, np.float64)
    ser_in, ser_w = loops.backward(ins, [w], scans, g, np.float32)
    cases.assert_under_bar(gin, want_in, cases.figures(ser_in, want_in)[0], "one plane, x and y: grad_in")
    cases.assert_under_bar(gw, want_w, cases.figures(ser_w, want_w)[0], "one plane, x and y: grad_w")
    assert gw[0][0, 0] == 0.0
    assert np.abs(gw[0][0, 1:]).max() > 0 and np.abs(gw[0][1:, 0]).max() > 0      # row 0 from the x scans, column 0 from the y scan


def test_a_null_entry_leaves_its_plane_untouched():
    import torch
    shape, planes = (70, 260), 1
    ins, ws = cases.case(shape, planes)
    g = cases.grad_out(shape, planes)
    both_in, both_w = run_backward(shape, planes, ALL, ins, ws, g, True)
    pattern = torch.arange(shape[0] * shape[1], dtype=torch.float32).view(shape)
    # the two gradient planes side by side in one guarded allocation; the x weights' plane holds a pattern and is NOT passed
    d_gw, g_gw = guarded.guarded_planes(shape, np.float32, 2, fill=guarded.OUT_FILL)
    d_gw[0].copy_(pattern)
    with rfa.VarPlan(shape, ALL, planes=planes, n_weights=2) as plan:
        gin, gw, times = plan.backward_timed(to_device(ins), to_device(ws), to_device(g), None, [None, d_gw[1]])
        torch.cuda.synchronize()
        assert gw[0] is None
        g_gw.check_guards("weight gradients")
        np.testing.assert_array_equal(bits(d_gw[0].cpu().numpy()), bits(pattern.numpy()))
        np.testing.assert_array_equal(bits(d_gw[1].cpu().numpy()), bits(both_w[1]))
        np.testing.assert_array_equal(bits(gin[0].cpu().numpy()), bits(both_in[0]))
        assert [n for n, _ in times] == (["var_tails_x", "var_carry", "var_pass2_x"] * 2 + ["var_tails_y", "var_carry", "var_pass2_y"] * 2
                                         + ["var_adj_tails_y", "var_carry", "var_adj_pass2_y", "var_grad_y"] * 2
                                         + ["var_adj_tails_x", "var_carry", "var_adj_pass2_x", "var_grad_x"] * 2)
        # the launches of the plane without a gradient are skipped
        assert all(ms == 0.0 for n, ms in times if n == "var_grad_x") and all(ms > 0.0 for n, ms in times if n == "var_grad_y")
    # a plane that is passed but that no scan reads is left as it is, too
    with rfa.VarPlan(shape, [PY, MY], planes=planes, n_weights=2) as plan:
        plan.backward(to_device(ins), to_device(ws), to_device(g), None, [d_gw[0], d_gw[1]])
        torch.cuda.synchronize()
    g_gw.check_guards("weight gradients")
    np.testing.assert_array_equal(bits(d_gw[0].cpu().numpy()), bits(pattern.numpy()))


# ---- guarded planes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,planes", [((70, 260), 1), ((130, 132), 3)])
def test_guarded_planes(shape, planes):
    import torch
    ins, ws = cases.case(shape, planes)
    g = cases.grad_out(shape, planes)
    d_in, g_in = guarded.guarded_planes(shape, np.float32, planes, fill=guarded.IN_FILL)
    d_w, g_w = guarded.guarded_planes(shape, np.float32, 2, fill=guarded.IN_FILL)
    d_g, g_g = guarded.guarded_planes(shape, np.float32, planes, fill=guarded.IN_FILL)
    d_gin, g_gin = guarded.guarded_planes(shape, np.float32, planes, fill=guarded.OUT_FILL)
    d_gw, g_gw = guarded.guarded_planes(shape, np.float32, 2, fill=guarded.OUT_FILL)
    for checker, arrays in ((g_in, ins), (g_w, ws), (g_g, g)):
        checker.load([torch.from_numpy(np.array(a)) for a in arrays])
        checker.snapshot()
    with rfa.VarPlan(shape, ALL, planes=planes, n_weights=2) as plan:
        plan.backward(d_in, d_w, d_g, d_gin, d_gw)
        torch.cuda.synchronize()
    g_gin.check_guards("grad_in")
    g_gw.check_guards("weight gradients")
    g_in.check_unchanged("input")
    g_w.check_unchanged("weights")
    g_g.check_unchanged("grad_out")
    cases.assert_gradients(host(d_gin), host(d_gw), shape, planes, "+x-x+y-y", f"guarded {shape} x {planes}")


# ---- argument checks that need a device -----------------------------------------------------------------------------------------
def test_backward_refusals():
    import torch
    shape = (40, 64)
    n = shape[0] * shape[1]
    new = lambda: torch.zeros(shape, device="cuda")      # noqa: E731
    x, w, g = new(), torch.full(shape, 0.5, device="cuda"), new()
    big = torch.zeros(2 * n + 8, device="cuda")
    off = big[1:1 + n].view(shape)                       # 4 bytes off a 16-byte boundary
    first, second = big[:n].view(shape), big[n // 2:n // 2 + n].view(shape)      # two aligned planes, half on top of each other
    with rfa.VarPlan(shape, [PX], planes=1, n_weights=1) as plan, rfa.VarPlan(shape, [PX], planes=2, n_weights=1) as two:
        def refused(p, text, *args):
            with pytest.raises(rfa.RecFilterError) as e:
                p.backward(*args)
            assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG and text in str(e.value), str(e.value)
        refused(plan, "in_planes", None, [w], [g], None, [new()])
        refused(plan, "plane 0: the varying scans need 16-byte aligned image pointers", [x], [w], [off], None, None)
        refused(plan, "plane 0: the varying scans need 16-byte aligned image pointers", None, [w], [g], [off], None)
        refused(plan, "weight plane 0: the varying scans need 16-byte aligned pointers", [x], [w], [g], None, [off])
        refused(plan, "grad_in plane 0 overlaps weight plane 0", [x], [w], [g], [w], None)
        refused(plan, "gradient of weight plane 0 overlaps weight plane 0", [x], [w], [g], None, [w])
        refused(plan, "grad_in plane 0 overlaps input plane 0", [x], [w], [g], [x], None)
        refused(plan, "gradient of weight plane 0 overlaps input plane 0", [x], [w], [g], None, [x])
        refused(plan, "grad_in plane 0 overlaps gradient of weight plane 0", [x], [w], [g], [first], [second])
        refused(plan, "gradient of weight plane 0 overlaps grad_out plane 0", [x], [w], [g], None, [g])
        refused(plan, "grad_in plane 0 overlaps grad_out plane 0", [x], [w], [first], [second], None)      # its own, only partly
        refused(two, "grad_in plane 0 overlaps grad_in plane 1", None, [w], [g, new()], [first, second], None)
        g2 = new()
        refused(two, "grad_in plane 0 overlaps grad_out plane 1", None, [w], [g, g2], [g2, new()], None)   # another index, exactly
        plan.backward(None, [w], [g], [g])               # its own, exactly: in place
        _, _, times = plan.backward_timed([x], [w], [g], None, [new()])
        assert [n for n, _ in times] == ["var_tails_x", "var_carry", "var_pass2_x", "var_adj_tails_x", "var_carry", "var_adj_pass2_x", "var_grad_x"]
        _, _, times = plan.backward_timed(None, [w], [g])
        assert [n for n, _ in times] == ["var_adj_tails_x", "var_carry", "var_adj_pass2_x"]
        assert plan.backward_num_kernels(True) == 7 and plan.backward_num_kernels(False) == 3
        torch.cuda.synchronize()


# ---- autograd -------------------------------------------------------------------------------------------------------------------
def test_apply_is_execute_with_a_backward():
    import torch
    shape, planes = (130, 132), 3
    ins, ws = cases.case(shape, planes)
    g = cases.grad_out(shape, planes)
    with rfa.VarPlan(shape, ALL, planes=planes, n_weights=2) as plan:
        d_in, d_w = to_device(ins), to_device(ws)
        plain = plan.execute(d_in, d_w)
        assert all(o.grad_fn is None for o in plan.apply(d_in, d_w))
        leaves = [t.clone().requires_grad_(True) for t in d_in]
        wx = d_w[0].clone().requires_grad_(True)             # the x weights want a gradient, the y weights do not
        outs = plan.apply(leaves, [wx, d_w[1]])
        guarded.assert_bits_equal([o.detach().cpu() for o in outs], [o.cpu() for o in plain], "apply against execute")
        torch.autograd.backward(list(outs), to_device(g))
        torch.cuda.synchronize()
        assert d_w[1].grad is None
        want_in, want_w, err_in, err_w = cases.expected(shape, planes, "+x-x+y-y")
        cases.assert_under_bar(host([t.grad for t in leaves]), want_in, err_in, "apply grad_in")
        cases.assert_under_bar([wx.grad.cpu().numpy()], [want_w[0]], err_w[0], "apply grad_w[0]")
    # the functional form: the same numbers from a cached plan
    leaves2 = [t.clone().requires_grad_(True) for t in d_in]
    outs2 = rfa.var_scan(leaves2, d_w, ALL)
    torch.autograd.backward(list(outs2), to_device(g))
    torch.cuda.synchronize()
    guarded.assert_bits_equal([t.grad.cpu() for t in leaves2], [t.grad.cpu() for t in leaves], "var_scan against apply")
    rfa.var_scan(d_in, d_w, ALL)
    assert len([k for k in rfa.varscan._scan_plans if k[0] == shape]) == 1


def torch_filter(image, guide, sigma_s, sigma_r, iterations, dtype):
    """the domain-transform filter on the CPU in `dtype`, plain torch: Python loops over the scanned dimension, vectorised over
    the lines; differentiable by torch's autograd"""
    import torch

    def scan(v, w, causal):      # along the last dimension of (C, L, N); w: (L, N), element 0 never read
        n = v.shape[-1]
        cols, acc = [None] * n, torch.zeros_like(v[..., 0])
        for i in (range(n) if causal else range(n - 1, -1, -1)):
            j = i if causal else i + 1
            if j == 0 or j == n:
                acc = v[..., i]
            else:
                acc = (1 - w[:, j]) * v[..., i] + w[:, j] * acc
            cols[i] = acc
        return torch.stack(cols, dim=-1)
    v, gd = image.to(dtype), guide.to(dtype)
    ratio = sigma_s / sigma_r
    one_col, one_row = torch.ones_like(gd[0, :, :1]), torch.ones_like(gd[0, :1, :])
    dx = torch.cat([one_col, 1 + ratio * (gd[:, :, 1:] - gd[:, :, :-1]).abs().sum(0)], dim=1)
    dy = torch.cat([one_row, 1 + ratio * (gd[:, 1:, :] - gd[:, :-1, :]).abs().sum(0)], dim=0)
    for a_k in rfa.domain_transform_bases(sigma_s, iterations):
        wx, wy = torch.pow(torch.tensor(a_k, dtype=dtype), dx), torch.pow(torch.tensor(a_k, dtype=dtype), dy)
        v = scan(scan(v, wx, True), wx, False)
        v = scan(scan(v.transpose(1, 2), wy.t(), True), wy.t(), False).transpose(1, 2)
    return v


def test_edge_aware_smooth_is_differentiable():
    import torch
    C, H, W, K, sigma_s, sigma_r = 3, 24, 36, 2, 8.0, 0.6
    rng = np.random.default_rng(2018)
    image = torch.from_numpy((rng.random((C, H, W)) * 2 - 1).astype(np.float32))
    guide = torch.from_numpy((0.5 * rng.random((C, H, W)) + np.linspace(0, 1, W)).astype(np.float32))      # seeded, no ties
    assert (guide[:, :, 1:] != guide[:, :, :-1]).all() and (guide[:, 1:, :] != guide[:, :-1, :]).all()
    g_out = torch.from_numpy((rng.random((C, H, W)) * 2 - 1).astype(np.float32))

    def reference(dtype):
        im, gd = image.clone().to(dtype).requires_grad_(True), guide.clone().to(dtype).requires_grad_(True)
        torch_filter(im, gd, sigma_s, sigma_r, K, dtype).backward(g_out.to(dtype))
        return im.grad.numpy(), gd.grad.numpy()
    want = reference(torch.float64)
    serial = reference(torch.float32)
    d_im, d_gd = image.cuda().requires_grad_(True), guide.cuda().requires_grad_(True)
    out = rfa.edge_aware_smooth(d_im, guide=d_gd, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K)
    assert out.grad_fn is not None
    out.backward(g_out.cuda())
    torch.cuda.synchronize()
    for what, got, w, s in (("image", d_im.grad, want[0], serial[0]), ("guide", d_gd.grad, want[1], serial[1])):
        cases.assert_under_bar([got.cpu().numpy()], [w], cases.figures([s], [w])[0], f"edge_aware_smooth gradient, {what}")
    # the value does not depend on who asks for gradients, and without them the path is the parent's: execute, driven by hand
    plain = rfa.edge_aware_smooth(image.cuda(), guide=guide.cuda(), sigma_s=sigma_s, sigma_r=sigma_r, iterations=K)
    assert plain.grad_fn is None
    with torch.no_grad():
        muted = rfa.edge_aware_smooth(d_im, guide=d_gd, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K)
    assert muted.grad_fn is None
    by_hand = torch.empty((C, H, W), device="cuda")
    with rfa.VarPlan((H, W), ALL, planes=C, n_weights=2) as plan:
        src, outs = [image.cuda()[c] for c in range(C)], [by_hand[c] for c in range(C)]
        for wx, wy in rfa.domain_transform_weights(guide.cuda(), sigma_s, sigma_r, K):
            plan.execute(src, [wx, wy], outs)
            src = outs
        torch.cuda.synchronize()
    for what, t in (("with gradients", out.detach()), ("without", plain), ("under no_grad", muted)):
        guarded.assert_bits_equal([t.cpu()], [by_hand.cpu()], f"edge_aware_smooth {what} against execute driven by hand")
    # an image that guides itself: the gradient reaches it both ways
    self_guided = image.cuda().requires_grad_(True)
    rfa.edge_aware_smooth(self_guided, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K).backward(g_out.cuda())
    assert self_guided.grad is not None and not torch.isnan(self_guided.grad).any()
    # the forms that are not differentiable say so by carrying no grad_fn
    assert rfa.edge_aware_smooth(d_im, guide=guide.cuda(), sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, form="plan").grad_fn is None


# ---- the C++ front-end ----------------------------------------------------------------------------------------------------------
def test_cpp_frontend_varying_grad(tmp_path):
    """RecFilterVarying::gradient: the adjoint of +x -x +y -y on 70 x 260 against loops in the C++ file, under the bar above;
    compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_varying_grad.cpp")
    exe = str(tmp_path / "test_frontend_varying_grad")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "varying-grad-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
