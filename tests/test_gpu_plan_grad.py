"""rf_plan_backward on the GPU: the three routes against the f64 loops of tests/plan_grad_loops.py, the exact and structural
properties of a backward call, torch.autograd on top, and the C++ front-end.

Bars.  Plane gradients: rc.rel_err under the suite's 1e-4 (the transposed filter is a filter of the forward's family).  Coefficient
gradients: |got - want| / sum|terms| <= max(4 x the same figure of the f32 loops, 1e-6), the form and floor of
tests/test_gpu_var_grad.py.  Measured figures: the docstring of test_coefficient_gradients."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import guarded as gd
import plan_grad_loops as pgl
import ref_cases as rc
import recfilter_amd as rfa
from recfilter_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, Z, C, A = rc.X, rc.Y, rc.Z, rc.C, rc.A
XYZ = rc.REFERENCE_TESTS["test_generic_xyz"]["scans"]
BIQUAD = [(X, C, [0.5, 0.4, -0.1])]
ORDER5 = [(X, C, [0.2, 0.5, 0.2, 0.1, 0.05, 0.02])]


def _fused(name, **kw):
    case = rc.FUSED_CASES[name]
    return dict(shape=case["shape"], scans=case["scans"], clamped=case["clamped"], **kw)


CASES = {
    "generic_xy_zero": _fused("generic_xy_zero"),
    "partial_mixed_zero": _fused("partial_mixed_zero"),
    "odd_w_mixed_zero": _fused("odd_w_mixed_zero"),
    "sat": _fused("sat"),
    "gauss2_clamped": _fused("gauss2_clamped"),
    "partial_xy_gauss3_clamped": _fused("partial_xy_gauss3_clamped"),
    "odd_w_one_past_a_tile": _fused("odd_w_one_past_a_tile"),
    "bicubic_clamped_ty32": _fused("bicubic_clamped_ty32", planes=3),
    "partial_x_only_causal_then_anti": _fused("partial_x_only_causal_then_anti"),
    "partial_y_only_scans": _fused("partial_y_only_scans"),
    "signal_4096_zero": dict(shape=(4096,), scans=BIQUAD, clamped=False),
    "signal_4096_clamped": dict(shape=(4096,), scans=BIQUAD, clamped=True),
    "volume_zero": dict(shape=(40, 36, 64), scans=XYZ, clamped=False),
    "volume_clamped": dict(shape=(40, 36, 64), scans=XYZ, clamped=True),
    "order5_zero": dict(shape=(64, 512), scans=ORDER5, clamped=False),
    "pointwise_zero": dict(shape=(128, 512), scans=rc.xy_pm(rc.GAUSS2), clamped=False, prologue=(0.5, 0.25), epilogue=(-0.7, 1.7, 0.1)),
}
COEFF_CASES = [n for n, c in CASES.items() if len(c["shape"]) >= 2 and "prologue" not in c]


def _plan(case, **kw):
    return rfa.Plan(case["shape"], case["scans"], clamped=case["clamped"], planes=case.get("planes", 1),
                    prologue=case.get("prologue"), epilogue=case.get("epilogue"), **kw)


def _inputs(case, signed):
    """host planes: the images (seed 1234 + plane) and grad_out (seed 4321 + plane; minus 0.5 for the coefficient checks)"""
    P = case.get("planes", 1)
    xs = [rc.random_image(case["shape"], seed=1234 + p) for p in range(P)]
    gs = [rc.random_image(case["shape"], seed=4321 + p) - (np.float32(0.5) if signed else np.float32(0.0)) for p in range(P)]
    return xs, gs


@functools.lru_cache(maxsize=None)
def _reference(name, signed, dtype):
    """(grad_ins per plane, rows, mags) of the loops, the rows summed over the planes; computed once per (case, grad_out, type)"""
    case = CASES[name]
    xs, gs = _inputs(case, signed)
    gins, rows, mags = [], 0.0, 0.0
    for x, g in zip(xs, gs):
        gi, r, m = pgl.backward(x, case["scans"], case["clamped"], g, dtype, case.get("prologue"), case.get("epilogue"))
        gins.append(gi)
        rows, mags = rows + r, mags + m
    for a in gins + [rows, mags]:
        a.setflags(write=False)
    return gins, rows, mags


def _cuda(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _plane_error(case, got, want, g):
    """rc.rel_err; a pointwise case is a sum of terms that cancel: judged against their magnitudes, as the forward's tests do"""
    if "epilogue" not in case:
        return rc.rel_err(got, want)
    ps, (pf, pi, _) = case["prologue"][0], case["epilogue"]
    ft, _, _ = pgl.backward(np.zeros_like(g), case["scans"], case["clamped"], g, np.float64)        # F^T(g)
    return rc.rel_err(got, want, scale=abs(ps) * (np.abs(pf * ft) + np.abs(pi * g.astype(np.float64))))


def _guarded_backward(plan, case, gs, xs=None):
    """one backward on guarded planes: grad_out (and the inputs) unchanged, nothing written outside grad_in; host results"""
    import torch
    P, shape = len(gs), case["shape"]
    ins = gi = None
    if xs is not None:
        ins, gi = gd.guarded_planes(shape, np.float32, P, fill=gd.IN_FILL)
        gi.load(_cuda(xs))
        gi.snapshot()
    rows = []

    def run(gouts, gins):
        _, r = plan.backward(gouts, gins, inputs=ins, coeff_grads=xs is not None)
        rows.append(r)
    got = gd.guarded_execute(run, shape, np.float32, np.float32, _cuda(gs))
    if gi is not None:
        gi.check_unchanged("input")
    return [g.numpy() for g in got], (rows[0].cpu().numpy() if rows[0] is not None else None)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plane_gradients(name):
    """routes 1 (zero border) and 2 (clamped) against the f64 loops, on guarded planes"""
    case = CASES[name]
    _, gs = _inputs(case, False)
    want, _, _ = _reference(name, False, np.float64)
    with _plan(case) as plan:
        got, _ = _guarded_backward(plan, case, gs)
    for p, (o, w) in enumerate(zip(got, want)):
        err = _plane_error(case, o, w, gs[p])
        print(f"gpu_plan_grad plane {name}[{p}]: rel_err {err:.3e}")
        assert err < 1e-4, (name, p, err)


@pytest.mark.parametrize("name", COEFF_CASES)
def test_coefficient_gradients(name):
    """route 3: every coefficient gradient under max(4 x the f32 loops' figure, 1e-6) of sum|terms|; its grad_in under the plane
    bar and against route 1 / 2.

    Measured on an MI355X over these cases: the worst figure is 1.054e-7 (`sat`, scan 0, feed-forward), 19 x the f32 loops'
    5.7e-9 for that entry and 0.105 of the floor; the next is 9.8e-8 (`partial_xy_gauss3_clamped`), 0.55 x the loops' 1.8e-7.  The
    floor of 1e-6 decides every case.  Route 3's grad_in: at most 2.0e-5 against the f64 loops, 2.8e-5 against route 2."""
    case = CASES[name]
    xs, gs = _inputs(case, True)
    want_g, want_rows, mags = _reference(name, True, np.float64)
    _, rows32, _ = _reference(name, True, np.float32)
    with _plan(case) as plan:
        got_g, rows = _guarded_backward(plan, case, gs, xs)
        plain, _ = plan.backward(_cuda(gs))
        plain = [t.cpu().numpy() for t in plain]
    worst = 0.0
    for s, (_, _, coeff) in enumerate(case["scans"]):
        assert not rows[s, len(coeff):].any(), "entries past the order are 0"
        for j in range(len(coeff)):
            fig = abs(rows[s, j] - want_rows[s, j]) / mags[s, j]
            yard = abs(rows32[s, j] - want_rows[s, j]) / mags[s, j]
            bar = max(4.0 * yard, 1e-6)
            worst = max(worst, fig)
            print(f"gpu_plan_grad coeff {name} scan {s} c{j}: figure {fig:.3e}, f32 loops {yard:.3e}, bar {bar:.3e}, "
                  f"gradient/normaliser {abs(want_rows[s, j]) / mags[s, j]:.3e}")
            assert fig <= bar, (name, s, j, fig, yard)
    print(f"gpu_plan_grad coeff {name}: worst {worst:.3e}")
    for p, (o, w, q) in enumerate(zip(got_g, want_g, plain)):
        err, between = rc.rel_err(o, w), rc.rel_err(o, q.astype(np.float64))
        print(f"gpu_plan_grad route3 plane {name}[{p}]: rel_err {err:.3e}, against route 1/2 {between:.3e}")
        assert err < 1e-4 and between < 1e-4, (name, p, err, between)


# ---- exact and structural checks --------------------------------------------------------------------------------------------
EXACT = ["generic_xy_zero", "gauss2_clamped"]


def _bits(tensors):
    return [t.clone() for t in tensors]


@pytest.mark.parametrize("name", EXACT)
def test_calls_are_reproducible_and_stateless(name):
    """two calls give identical bits (planes and coefficients), also behind an unrelated plan's execute; a poisoned call in
    between leaves nothing behind; in place equals out of place"""
    import torch
    case = CASES[name]
    xs, gs = _inputs(case, True)
    x, g = _cuda(xs), _cuda(gs)
    with _plan(case) as plan, rfa.Plan((64, 256), rc.xy_pm(rc.GAUSS3), clamped=True) as other:
        for coeffs in (False, True):
            kw = dict(inputs=x, coeff_grads=True) if coeffs else {}
            a, ra = plan.backward(g, **kw)
            b, rb = plan.backward(g, **kw)
            gd.assert_bits_equal(a, b, f"{name}: second call")
            other.execute([torch.rand(64, 256, device="cuda")])
            c, rcf = plan.backward(g, **kw)
            gd.assert_bits_equal(a, c, f"{name}: behind another plan's execute")
            poison = [gd.nan_like(t).cuda() for t in g]
            plan.backward(poison, **kw)
            d, rd = plan.backward(g, **kw)
            gd.assert_bits_equal(a, d, f"{name}: behind a poisoned call")
            if coeffs:
                gd.assert_bits_equal([ra, ra, ra], [rb, rcf, rd], f"{name}: coefficient rows")
                assert bool(torch.isfinite(ra).all())
            inplace = _bits(g)
            out, _ = plan.backward(inplace, inplace, **kw)
            assert out[0].data_ptr() == inplace[0].data_ptr()
            gd.assert_bits_equal(a, out, f"{name}: in place")


@pytest.mark.parametrize("name", EXACT + ["volume_clamped"])
def test_launch_lists(name):
    """backward_num_kernels is the length of the timed list on every route; route 1 is the forward plan of the transposed
    scans, name for name, and needs no workspace; the adjoint kernels carry their fixed names"""
    case = CASES[name]
    xs, gs = _inputs(case, True)
    x, g = _cuda(xs), _cuda(gs)
    n = len(case["scans"])
    with _plan(case) as plan:
        _, _, plain = plan.backward_timed(g)
        _, rows, full = plan.backward_timed(g, inputs=x, coeff_grads=True)
        assert len(plain) == plan.backward_num_kernels(False) > 0
        assert len(full) == plan.backward_num_kernels(True) > len(plain)
        assert plan.backward_workspace_bytes(False) == 0
        assert plan.backward_workspace_bytes(True) == (n + 1) * 4 * int(np.prod(case["shape"])) + 1024 * 33 * 8
        names, full_names = [k for k, _ in plain], [k for k, _ in full]
        if not case["clamped"]:
            transposed = [(d, not c, w) for d, c, w in reversed(case["scans"])]
            with rfa.Plan(case["shape"], transposed, clamped=False) as t:
                _, fwd = t.execute_timed(g)
            assert names == [k for k, _ in fwd]
            assert "adjoint_border" not in full_names
        else:
            assert names.count("adjoint_border") == n and names[-1] == "adjoint_border"
            assert full_names.count("adjoint_border") == n
        assert full_names.count("coeff_grad") == n and full_names.count("coeff_grad_sum") == n
        for i, k in enumerate(full_names):
            if k == "coeff_grad":
                assert full_names[i + 1] == "coeff_grad_sum"
        assert rows.shape == (n, 1 + capi.RF_MAX_ORDER)


@pytest.mark.parametrize("name", EXACT)
def test_forward_is_untouched(name):
    """the execute of a plan gives the same bits, and the plan reports the same forward side, before and after its first backward"""
    case = CASES[name]
    xs, gs = _inputs(case, True)
    x, g = _cuda(xs), _cuda(gs)
    with _plan(case) as plan:
        before = plan.execute(x)
        state = (plan.workspace_bytes, plan.num_kernels, plan.debug_buffers(), plan.num_instances)
        applied = plan.apply(x)
        plan.backward(g)
        plan.backward(g, inputs=x, coeff_grads=True)
        after = plan.execute(x)
        gd.assert_bits_equal(before, after, f"{name}: execute after the backward")
        gd.assert_bits_equal(before, list(applied), f"{name}: Plan.apply")
        assert state == (plan.workspace_bytes, plan.num_kernels, plan.debug_buffers(), plan.num_instances)


@pytest.mark.parametrize("clamped", [False, True], ids=["zero", "clamped"])
@pytest.mark.parametrize("scan", [(X, C, [0.75, 0.0, 0.0]), (Y, A, [1.7, 0.0])], ids=["x_causal_order2", "y_anticausal_order1"])
def test_zero_feedback_is_exact(scan, clamped):
    """feedback of all zeros: grad_in is c0 g exactly (on every route), dL/dc0 the f64 dot product, the feedback rows finite"""
    shape = (64, 256)
    x, g = rc.random_image(shape, seed=1234), rc.random_image(shape, seed=4321) - np.float32(0.5)
    with rfa.Plan(shape, [scan], clamped=clamped) as plan:
        (plain,), _ = plan.backward(_cuda([g]))
        (full,), rows = plan.backward(_cuda([g]), inputs=_cuda([x]), coeff_grads=True)
    want = np.float32(scan[2][0]) * g
    assert np.array_equal(plain.cpu().numpy(), want) and np.array_equal(full.cpu().numpy(), want)
    rows = rows.cpu().numpy()
    dot = float(np.sum(g.astype(np.float64) * x.astype(np.float64)))
    assert abs(rows[0, 0] - dot) <= 1e-12 * abs(dot), (rows[0, 0], dot)
    assert np.isfinite(rows).all() and not rows[0, len(scan[2]):].any()


# ---- autograd ---------------------------------------------------------------------------------------------------------------
def test_plan_apply_autograd():
    import torch
    case = CASES["bicubic_clamped_ty32"]
    xs, gs = _inputs(case, True)
    g = _cuda(gs)
    with _plan(case) as plan:
        x = [t.requires_grad_(True) for t in _cuda(xs)]
        outs = plan.apply(x)
        gd.assert_bits_equal(list(outs), plan.execute([t.detach() for t in x]), "Plan.apply")
        assert all(o.grad_fn is not None for o in outs)
        grads = torch.autograd.grad(outs, x, g)
        want, _ = plan.backward(g)
        gd.assert_bits_equal(list(grads), want, "autograd through Plan.apply")


def test_recursive_filter_autograd():
    """torch.autograd.grad through recursive_filter gives the backward's tensors; the four scans of a Gaussian share one
    coefficient tensor whose gradient is the sum of the four rows"""
    import torch
    shape = (128, 512)
    x = rc.cuda_image(shape).requires_grad_(True)
    g = rc.cuda_image(shape, seed=4321) - 0.5
    w = torch.tensor(rc.GAUSS2, dtype=torch.float64, device="cuda", requires_grad=True)
    b = torch.tensor([0.9, 0.05], dtype=torch.float32, requires_grad=True)             # a host tensor, another type
    dirs = [(X, C), (X, A), (Y, C), (Y, A), (X, C)]
    out = rfa.recursive_filter(x, dirs, [w, w, w, w, b], clamped=True)
    assert out.grad_fn is not None
    scans = [(d, c, rc.GAUSS2) for d, c in dirs[:4]] + [(X, C, [0.9, 0.05])]
    with rfa.Plan(shape, scans, clamped=True) as plan:
        assert gd.bits_equal(out.detach(), plan.execute([x.detach()])[0])
        (want_x,), rows = plan.backward([g], inputs=[x.detach()], coeff_grads=True)
    gx, gw, gb = torch.autograd.grad(out, [x, w, b], g)
    assert gd.bits_equal(gx, want_x)
    assert gw.dtype == torch.float64 and gw.is_cuda and torch.allclose(gw, rows[:4, :3].sum(dim=0), rtol=1e-14, atol=0.0)
    assert gb.dtype == torch.float32 and not gb.is_cuda and torch.equal(gb, rows[4, :2].float().cpu())
    # the image alone: no coefficient pass
    (gx2,) = torch.autograd.grad(rfa.recursive_filter(x, dirs, [w.detach()] * 4 + [b.detach()], clamped=True), [x], g)
    with rfa.Plan(shape, scans, clamped=True) as plan:
        gd.assert_bits_equal([gx2], plan.backward([g])[0], "image gradient alone")


def test_recursive_filter_cache_evicts_and_closes():
    import torch
    from recfilter_amd import plan as plan_module
    plan_module._filter_plans.clear()
    x = rc.cuda_image((32, 64))
    first = None
    for i in range(plan_module.FILTER_PLAN_CACHE + 1):
        rfa.recursive_filter(x, [(X, C)], [torch.tensor([0.5, 0.25 + i / 64.0])])
        if first is None:
            (first,) = plan_module._filter_plans.values()
            assert first._h
    assert len(plan_module._filter_plans) == plan_module.FILTER_PLAN_CACHE
    assert not first._h, "the evicted plan is closed"
    assert first not in plan_module._filter_plans.values()
    # the same values again: one plan, found by value
    rfa.recursive_filter(x, [(X, C)], [torch.tensor([0.5, 0.5])])
    n = len(plan_module._filter_plans)
    rfa.recursive_filter(x, [(X, C)], [torch.tensor([0.5, 0.5], dtype=torch.float64)])
    assert len(plan_module._filter_plans) == n


# ---- C++ --------------------------------------------------------------------------------------------------------------------
def test_cpp_frontend_gradient(tmp_path):
    """RecFilter::gradient against rf_plan_backward, bit for bit; compiled here with the command line of
    test_gpu_smooth_batch.py::test_cpp_frontend_smooth_batch"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_gradient.cpp")
    exe = str(tmp_path / "test_frontend_gradient")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "gradient-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
