"""GPU tests of the bases' gradient of the power form (rf_var_plan_backward_power_bases: the base-reducing var_grad instances and
var_param_sum of kernels_var.hip, plan_var.cpp, VarPlan.backward_power_bases / VarPlan.apply_power / smooth_samples of
recfilter_amd/varscan.py).

Reference: the f64 loops of tests/sigma_grad_loops.py (pinned against central differences by tests/test_sigma_grad_host.py).  Bar,
for every scalar: |got - want_f64| / sum |terms| <= max(4 x the same figure of the f32 serial loops, 1e-6), the bar of
tests/test_gpu_plan_grad.py::test_coefficient_gradients; every figure is printed.  The planes a call also writes are bit for bit
those of backward_power, and two calls agree bit for bit."""
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import guarded
import sigma_grad_loops as gloops
import var_grad_cases as vcases
import recfilter_amd as rfa
from smooth_volume_grad_loops import SCANS as VOLUME_SCANS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = vcases.SCAN_LISTS["+x-x+y-y"]
PAIR_1D = [(0, True, 0), (0, False, 0)]
BASES = [0.9, 0.8, 0.85]

# name: (kind, shape, planes, scans, exponent planes, sprinkled).  (70, 132): partial tiles both ways; (3, 1028): the second workgroup
# along x holds one live lane; (65540, 4): taller than the 65535 rows of the grid, the stride loop of either grid (the reducing form walks 1024 rows at once); 12616: 13 workgroups, the last partial
CASES = {
    "1x4": ("image", (1, 4), 1, ALL, 2, False),
    "70x132": ("image", (70, 132), 2, ALL, 2, False),
    "3x1028": ("image", (3, 1028), 1, ALL, 2, False),
    "65540x4": ("image", (65540, 4), 1, ALL, 2, False),
    "signal4": ("signal", (4,), 1, PAIR_1D, 1, False),
    "signal12616": ("signal", (12616,), 2, PAIR_1D, 1, False),
    "volume": ("volume", (6, 10, 12), 2, VOLUME_SCANS, 3, False),
    "sprinkled": ("image", (70, 132), 2, ALL, 2, True),
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(ins, exponents, grad_outs) of a case, seeded, f32, never written.  Exponents 1 .. 4 with NaN at element 0 along the dimension
    their scans run along; sprinkled: +inf and 0 at 5 % each"""
    kind, shape, planes, scans, n_exp, sprinkled = CASES[name]
    rng = np.random.default_rng(zlib.crc32(repr((name, "sigma grad")).encode()))
    ins = [(rng.random(shape) * 2 - 1).astype(np.float32) for _ in range(planes)]
    g = [(rng.random(shape) * 2 - 1).astype(np.float32) for _ in range(planes)]
    ds = [(1.0 + 3.0 * rng.random(shape)).astype(np.float32) for _ in range(n_exp)]
    for d in ds:
        if sprinkled:
            u = rng.random(shape)
            d[u < 0.05] = np.inf
            d[u > 0.95] = 0.0
    for dim, _, k in scans:
        first = [slice(None)] * len(shape)
        first[len(shape) - 1 - dim] = 0
        ds[k][tuple(first)] = np.nan
    for a in ins + g + ds:
        a.setflags(write=False)
    return ins, ds, g


@functools.lru_cache(maxsize=None)
def expected(name):
    """(f64 dL/dbases, the f32 loops' figures, the normalisers)"""
    _, _, _, scans, n_exp, _ = CASES[name]
    ins, ds, g = inputs(name)
    _, want, norms = gloops.power_bases_backward(ins, ds, BASES[:n_exp], scans, g, np.float64)
    _, ser, _ = gloops.power_bases_backward(ins, ds, BASES[:n_exp], scans, g, np.float32)
    return want, [gloops.figure(s, w, n) for s, w, n in zip(ser, want, norms)], norms


def make_plan(name):
    kind, shape, planes, scans, n_exp, _ = CASES[name]
    if kind == "signal":
        return rfa.VarPlan.signal(shape[0], scans, planes=planes, n_weights=n_exp)
    if kind == "volume":
        return rfa.VarPlan.volume(shape, scans, planes=planes, n_weights=n_exp)
    return rfa.VarPlan(shape, scans, planes=planes, n_weights=n_exp)


def device(arrays):
    import torch
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]


def nan_planes(like, n):
    import torch
    return [torch.full(like.shape, float("nan"), device="cuda") for _ in range(n)]


def assert_scalars(got, name, what):
    want, yards, norms = expected(name)
    assert np.isfinite(got).all(), (what, got)
    for k, (v, w, yard, n) in enumerate(zip(got, want, yards, norms)):
        fig = gloops.figure(v, w, n)
        print(f"gpu_sigma_grad {what} base {k}: got {v:.9e}, want {w:.9e}, figure {fig:.3e}, f32 loops {yard:.3e}, bar {gloops.bar(yard):.3e}, "
              f"gradient/normaliser {abs(w) / n if n else 0.0:.3e}")
        assert fig <= gloops.bar(yard), (what, k, fig, yard)


# ---- parity and bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_base_gradients(name):
    import torch
    n_exp = CASES[name][4]
    bases = BASES[:n_exp]
    ins, ds, g = (device(a) for a in inputs(name))
    with make_plan(name) as plan:
        ref_in, ref_d = plan.backward_power(ins, ds, bases, g, None, nan_planes(ins[0], n_exp))
        gin, gd, gb = plan.backward_power_bases(ins, ds, bases, g, None, nan_planes(ins[0], n_exp))
        # no exponent gradient at all, and only the last plane's: the same scalars and the same planes
        gin_none, none, gb_none = plan.backward_power_bases(ins, ds, bases, g)
        some = [None] * (n_exp - 1) + nan_planes(ins[0], 1)
        gin_some, gd_some, gb_some = plan.backward_power_bases(ins, ds, bases, g, None, some)
        torch.cuda.synchronize()
    assert none is None and gb.dtype == torch.float64 and tuple(gb.shape) == (n_exp,)
    assert_scalars(gb.cpu().numpy(), name, name)
    guarded.assert_bits_equal(gin + gd, ref_in + ref_d, f"{name}: grad_in and grad_exponents against backward_power")
    guarded.assert_bits_equal(gin_none + gin_some + [gd_some[-1]], ref_in + ref_in + [ref_d[-1]], f"{name}: planes with exponent gradients left out")
    guarded.assert_bits_equal([gb_none, gb_some], [gb, gb], f"{name}: scalars with exponent gradients left out")
    if CASES[name][5]:
        assert not any(torch.isnan(t).any() for t in gin + gd)


def test_a_plane_no_scan_reads_gets_zero():
    import torch
    shape = (70, 132)
    ins, ds, g = (device(a) for a in inputs("70x132"))
    d = ds[0].clone()
    d[:, 0] = d[:, 1]                                  # column 0 is read by the y scan, row 0 by the x scan:
    d[0, 0] = float("nan")                             # the one element neither reads
    with rfa.VarPlan(shape, [(0, True, 0), (1, False, 0)], planes=2, n_weights=2) as plan:
        _, _, gb = plan.backward_power_bases(ins, [d, ds[1]], [0.9, 0.8], g, None, None, torch.full((2,), float("nan"), dtype=torch.float64, device="cuda"))
    got = gb.cpu().numpy()
    assert np.isfinite(got[0]) and got[0] != 0.0 and got[1] == 0.0


# ---- reproducible, stateless -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["70x132", "volume", "signal12616"])
def test_two_calls_agree_bit_for_bit(name):
    """also with an unrelated plan's execute between them, and with a call on NaN planes between them -- which leaves NaN in every
    plane and every slab the plan owns (the varying plans have no debug fill: this is how their tests poison scratch)"""
    import torch
    n_exp = CASES[name][4]
    bases = BASES[:n_exp]
    ins, ds, g = (device(a) for a in inputs(name))
    other_in, other_w = device([np.ones((40, 64), dtype=np.float32)]), device([np.full((40, 64), 0.5, dtype=np.float32)] * 2)
    with make_plan(name) as plan, rfa.VarPlan((40, 64), ALL, planes=1, n_weights=2) as other:
        results = []
        for step in range(3):
            gin, gd, gb = plan.backward_power_bases(ins, ds, bases, g, None, nan_planes(ins[0], n_exp))
            results.append([t.clone() for t in gin + gd + [gb]])
            if step == 0:
                other.execute(other_in, other_w)
            else:
                poison = nan_planes(ins[0], len(ins))
                _, _, poisoned = plan.backward_power_bases(poison, ds, bases, poison, None, nan_planes(ins[0], n_exp))
                assert torch.isnan(poisoned).all()
        torch.cuda.synchronize()
    assert np.isfinite(results[0][-1].cpu().numpy()).all()
    for r in results[1:]:
        guarded.assert_bits_equal(r, results[0], f"{name}: repeated calls of one plan")


# ---- launch lists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["70x132", "volume", "signal12616"])
def test_timed_names_and_counts(name):
    n_exp = CASES[name][4]
    bases = BASES[:n_exp]
    ins, ds, g = (device(a) for a in inputs(name))
    with make_plan(name) as plan:
        _, _, with_planes = plan.backward_power_timed(ins, ds, bases, g, None, nan_planes(ins[0], n_exp))
        _, _, gb, timings = plan.backward_power_bases_timed(ins, ds, bases, g)
        assert len(timings) == plan.backward_bases_num_kernels() == 7 * len(CASES[name][3]) + 1
        assert [n for n, _ in timings] == [n for n, _ in with_planes] + ["var_param_sum"]
    assert_scalars(gb.cpu().numpy(), name, f"{name} timed")


# ---- guarded planes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["70x132", "3x1028", "signal12616", "volume"])
def test_guarded_planes(name):
    """nothing is read outside the caller's planes (NaN guards) and nothing written outside the gradient planes and the 8-byte
    aligned result buffer"""
    import torch
    kind, shape, planes, scans, n_exp, _ = CASES[name]
    bases = BASES[:n_exp]
    ins, ds, g = inputs(name)
    roles = []
    for arrays in (ins, ds, g):
        views, checker = guarded.guarded_planes(shape, np.float32, len(arrays), fill=guarded.IN_FILL)
        checker.load([torch.from_numpy(np.array(a)) for a in arrays])
        checker.snapshot()
        roles.append((views, checker))
    gin, c_gin = guarded.guarded_planes(shape, np.float32, planes)
    gd, c_gd = guarded.guarded_planes(shape, np.float32, n_exp)
    gb, c_gb = guarded.guarded_planes((n_exp,), np.float64, 1)
    with make_plan(name) as plan:
        plan.backward_power_bases(roles[0][0], roles[1][0], bases, roles[2][0], gin, gd, gb[0])
        torch.cuda.synchronize()
        for checker, what in ((c_gin, "grad_in"), (c_gd, "grad_exponents"), (c_gb, "grad_bases")):
            checker.check_guards(what)
        for (_, checker), what in zip(roles, ("input", "exponent", "grad_out")):
            checker.check_unchanged(what)
        ref_in, ref_d = plan.backward_power(device(ins), device(ds), bases, device(g), None, nan_planes(gin[0], n_exp))
        torch.cuda.synchronize()
    assert_scalars(gb[0].cpu().numpy(), name, f"{name} guarded")
    guarded.assert_bits_equal(gin + gd, ref_in + ref_d, f"{name}: guarded planes against backward_power")


def test_run_refusals():
    import torch
    ins, ds, g = (device(a) for a in inputs("70x132"))
    with make_plan("70x132") as plan:
        raw = torch.empty(4, dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError, match="grad_bases"):
            plan.backward_power_bases(ins, ds, BASES[:2], g, None, None, raw)                       # four entries for two planes
        with pytest.raises(ValueError, match="grad_bases"):
            plan.backward_power_bases(ins, ds, BASES[:2], g, None, None, raw[:2].float())
        with pytest.raises(rfa.RecFilterError, match="overlaps"):
            plan.backward_power_bases(ins, ds, BASES[:2], g, None, [ins[0], None])


# ---- autograd ----------------------------------------------------------------------------------------------------------------------
def test_apply_power_with_tensor_bases():
    import torch
    name = "70x132"
    ins, ds, g = (device(a) for a in inputs(name))
    with make_plan(name) as plan:
        bases = torch.tensor(BASES[:2], dtype=torch.float64, requires_grad=True)      # (a host tensor: its gradient comes back to the host)
        d0 = ds[0].clone().requires_grad_(True)
        outs = plan.apply_power(ins, [d0, ds[1]], bases)
        torch.autograd.backward(outs, g)
        constant = plan.apply_power(ins, ds, BASES[:2])
        ref_in, ref_d = plan.backward_power(ins, ds, BASES[:2], g, None, nan_planes(ins[0], 2))
        torch.cuda.synchronize()
    guarded.assert_bits_equal(list(outs), list(constant), "values with tensor bases against float bases")
    guarded.assert_bits_equal([d0.grad], [ref_d[0]], "the exponent gradient beside the bases' gradient")
    assert bases.grad.dtype == torch.float64 and bases.grad.shape == bases.shape and not bases.grad.is_cuda
    assert_scalars(bases.grad.numpy(), name, "apply_power")
    # bases that need no gradient take backward_power: nothing comes back for them
    fixed = torch.tensor(BASES[:2], dtype=torch.float32)
    d1 = ds[1].clone().requires_grad_(True)
    with make_plan(name) as plan:
        torch.autograd.backward(plan.apply_power(ins, [ds[0], d1], fixed), g)
        torch.cuda.synchronize()
    guarded.assert_bits_equal([d1.grad], [ref_d[1]], "tensor bases without a gradient")
    assert fixed.grad is None


@pytest.mark.parametrize("zero_phase", [True, False])
def test_smooth_samples_with_a_tensor_time_constant(zero_phase):
    import torch
    n, tau = 12614, 3.0                                  # (not a multiple of 4: padded with gaps of +inf)
    rng = np.random.default_rng(2810)
    x = rng.random((2, n)) * 2 - 1
    gaps = 0.2 + 2.0 * rng.random(n)
    g = rng.random((2, n)) * 2 - 1
    t = torch.tensor(tau, dtype=torch.float64, requires_grad=True)
    dx = torch.from_numpy(x.astype(np.float32)).cuda()
    dgaps = torch.from_numpy(gaps.astype(np.float32)).cuda()
    y = rfa.smooth_samples(dx, dgaps, t, zero_phase=zero_phase)
    y.backward(torch.from_numpy(g.astype(np.float32)).cuda())
    y_float = rfa.smooth_samples(dx, dgaps, tau, zero_phase=zero_phase)
    assert guarded.bits_equal(y.detach(), y_float)
    base = float(np.float32(np.exp(-1.0 / tau)))
    scans = PAIR_1D if zero_phase else PAIR_1D[:1]
    args = ([r.astype(np.float32) for r in x], [gaps.astype(np.float32)], [base], scans, [r.astype(np.float32) for r in g])
    _, want, norms = gloops.power_bases_backward(*args, np.float64)
    _, ser, _ = gloops.power_bases_backward(*args, np.float32)
    chain = np.exp(-1.0 / tau) / tau ** 2                # d base / d tau
    fig = abs(t.grad.item() - want[0] * chain) / (norms[0] * chain)
    bar = gloops.bar(gloops.figure(ser[0], want[0], norms[0]))
    print(f"gpu_sigma_grad smooth_samples zero_phase={zero_phase}: dL/dtau {t.grad.item():.9e}, want {want[0] * chain:.9e}, figure {fig:.3e}, bar {bar:.3e}")
    assert fig <= bar


# ---- the C++ front-end -------------------------------------------------------------------------------------------------------------
def test_cpp_frontend_sigma_grad(tmp_path):
    """RecFilterVarying::gradient_power_bases against f64 loops in the C++ file, under the bar above; compiled here with the command
    line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_sigma_grad.cpp")
    exe = str(tmp_path / "test_frontend_sigma_grad")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "sigma-grad-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])


# ---- rf_smooth_plan_set_sigmas -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["image", "batch", "volume"])
def test_set_sigmas_runs_as_a_fresh_plan(kind):
    """execute and backward after set_sigmas are bit for bit those of a plan created with the new sigmas; the plan keeps its
    workspace"""
    import torch
    rng = np.random.default_rng(2812)
    shape = {"image": (3, 70, 132), "batch": (2, 3, 70, 132), "volume": (2, 6, 10, 12)}[kind]
    image = torch.from_numpy(rng.random(shape).astype(np.float32)).cuda()
    g = torch.from_numpy((rng.random(shape) * 2 - 1).astype(np.float32)).cuda()

    def make(sigma_s, sigma_r):
        if kind == "volume":
            return rfa.SmoothPlan.volume(shape[1:], planes=shape[0], iterations=2, sigma_s=sigma_s, sigma_r=sigma_r, spacing_z=2.5, differentiable=True)
        return rfa.SmoothPlan(shape[-2:], planes=shape[-3], iterations=2, sigma_s=sigma_s, sigma_r=sigma_r, batch=shape[0] if kind == "batch" else None)

    def run(plan):
        out = plan.execute(image, None)
        grads = plan.backward(image, None, g, edges=True)
        torch.cuda.synchronize()
        return [out.clone(), grads[0].clone()]
    with make(3.0, 0.8) as plan, make(9.5, 0.3) as fresh:
        first = run(plan)
        workspace = plan.workspace_bytes
        plan.set_sigmas(9.5, 0.3)
        assert plan.bases == fresh.bases and plan.workspace_bytes == workspace
        retuned, want = run(plan), run(fresh)
        guarded.assert_bits_equal(retuned, want, f"{kind}: after set_sigmas against a fresh plan")
        assert not guarded.bits_equal(retuned[0], first[0]), "the new sigmas change the result"
        plan.set_sigmas(3.0, 0.8)
        guarded.assert_bits_equal(run(plan), first, f"{kind}: back to the first sigmas")


# ---- rf_smooth_plan_backward_sigmas -------------------------------------------------------------------------------------------------
import smooth_grad_cases as scases      # noqa: E402

SIGMA_S, SIGMA_R = scases.SIGMA_S, scases.SIGMA_R
SMOOTH_SHAPE = (3, 70, 132)
VOLUME_SHAPE = (2, 6, 10, 12)


def volume_arrays(channels=None):
    rng = np.random.default_rng(2813)
    C = VOLUME_SHAPE[0] if channels is None else channels
    ramps = sum(np.linspace(0, 1, n).reshape([-1 if i == ax else 1 for i in range(4)]) for ax, n in enumerate(VOLUME_SHAPE) if ax > 0)
    guide = (0.5 * rng.random((C,) + VOLUME_SHAPE[1:]) + ramps).astype(np.float32)
    return (rng.random(VOLUME_SHAPE).astype(np.float32), guide, (rng.random(VOLUME_SHAPE) * 2 - 1).astype(np.float32))


@functools.lru_cache(maxsize=None)
def smooth_expected(K, self_guided, kind="image"):
    """(f64 params, the f32 loops' figures, normalisers) of the 3 + K scalars"""
    if kind == "volume":
        image, guide, g = volume_arrays(1)
        args, sz, byte = (image, None if self_guided else guide, SIGMA_S, SIGMA_R, K, g), 2.5, False
    elif kind == "bytes":
        image, g = scases.image(SMOOTH_SHAPE), scases.grad_out(SMOOTH_SHAPE)
        args, sz, byte = (image, byte_guide().astype(np.float32), SIGMA_S, SIGMA_R, K, g), None, True
    else:
        image, g = scases.image(SMOOTH_SHAPE), scases.grad_out(SMOOTH_SHAPE)
        args, sz, byte = (image, None if self_guided else scases.guide(SMOOTH_SHAPE, 1), SIGMA_S, SIGMA_R, K, g), None, False
    want, norms = gloops.smooth_sigma_backward(*args, np.float64, sz, byte_guide=byte)
    ser, _ = gloops.smooth_sigma_backward(*args, np.float32, sz, byte_guide=byte)
    return want, [gloops.figure(s_, w, n) for s_, w, n in zip(ser, want, norms)], norms


def byte_guide():
    return np.clip(np.rint(scases.guide(SMOOTH_SHAPE, 1) * 100.0), 0, 255).astype(np.uint8)


def assert_params(got, expected_, what):
    want, yards, norms = expected_
    assert len(got) == len(want) and np.isfinite(got).all(), (what, got)
    names = ["sigma_s", "sigma_r", "spacing_z"] + [f"a_{k}" for k in range(len(want) - 3)]
    for v, w, yard, n, name in zip(got, want, yards, norms, names):
        fig = gloops.figure(v, w, n)
        print(f"gpu_sigma_grad {what} {name}: got {v:.9e}, want {w:.9e}, figure {fig:.3e}, f32 loops {yard:.3e}, bar {gloops.bar(yard):.3e}")
        assert fig <= gloops.bar(yard), (what, name, fig, yard)


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


@pytest.mark.parametrize("edges", [False, True])
@pytest.mark.parametrize("self_guided", [True, False])
@pytest.mark.parametrize("K", [2, 3])
def test_smooth_sigma_gradients(K, self_guided, edges):
    import torch
    image, g = cuda(scases.image(SMOOTH_SHAPE)), cuda(scases.grad_out(SMOOTH_SHAPE))
    guide = None if self_guided else cuda(scases.guide(SMOOTH_SHAPE, 1))
    with rfa.SmoothPlan(SMOOTH_SHAPE[1:], planes=3, guide_planes=0 if self_guided else 1, iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R) as plan:
        ref = plan.backward(image, guide, g, edges=edges)
        ref = [t.clone() for t in ref if t is not None]
        gi, gg, gp = plan.backward_sigmas(image, guide, g, edges=edges)
        first = [gi.clone(), gp.clone()] + ([gg.clone()] if gg is not None else [])
        gi2, gg2, gp2, timings = plan.backward_sigmas_timed(image, guide, g, edges=edges)
        torch.cuda.synchronize()
        assert len(timings) == plan.backward_sigmas_num_kernels(edges) == 34 * K - (2 if edges else 3)
        assert [n for n, _ in timings][-2:] == ["var_dot", "var_param_sum"]
    what = f"smooth K={K} {'self-guided' if self_guided else 'guided'} edges={int(edges)}"
    assert_params(gp.cpu().numpy(), smooth_expected(K, self_guided), what)
    guarded.assert_bits_equal([gi] + ([gg] if gg is not None else []), ref, what + ": grad_image and grad_guide against backward")
    guarded.assert_bits_equal([gi2, gp2] + ([gg2] if gg2 is not None else []), first, what + ": two calls")


def test_smooth_sigma_gradients_of_a_batch_are_the_sum_over_its_images():
    import torch
    K, N = 2, 3
    rng = np.random.default_rng(2814)
    base_image, base_g = scases.image(SMOOTH_SHAPE), scases.grad_out(SMOOTH_SHAPE)
    images = np.stack([np.roll(base_image, 7 * b, axis=2) * (1.0 - 0.2 * b) for b in range(N)]).astype(np.float32)
    gs = np.stack([np.roll(base_g, 5 * b, axis=1) for b in range(N)]).astype(np.float32)
    common = dict(planes=3, iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R)
    with rfa.SmoothPlan(SMOOTH_SHAPE[1:], batch=N, **common) as batched, rfa.SmoothPlan(SMOOTH_SHAPE[1:], **common) as single:
        _, _, gp = batched.backward_sigmas(cuda(images), None, cuda(gs), edges=True)
        singles = [single.backward_sigmas(cuda(images[b]), None, cuda(gs[b]), edges=True)[2].clone() for b in range(N)]
        torch.cuda.synchronize()
    want = [np.zeros(3 + K), [0.0] * (3 + K), np.zeros(3 + K)]
    for b in range(N):
        w, _, n = (lambda r: (r[0], None, r[1]))(gloops.smooth_sigma_backward(images[b], None, SIGMA_S, SIGMA_R, K, gs[b], np.float64))
        s32, _ = gloops.smooth_sigma_backward(images[b], None, SIGMA_S, SIGMA_R, K, gs[b], np.float32)
        want[0] += np.array(w, dtype=np.float64)
        want[2] += np.array(n)
        want[1] = [y + abs(float(a) - float(c)) for y, a, c in zip(want[1], s32, w)]
    yards = [y / n if n else 0.0 for y, n in zip(want[1], want[2])]
    assert_params(gp.cpu().numpy(), (list(want[0]), yards, list(want[2])), "smooth batch of 3")
    total = sum(t.cpu().numpy() for t in singles)
    assert_params(gp.cpu().numpy(), (list(total), yards, list(want[2])), "smooth batch of 3 against three single calls")


@pytest.mark.parametrize("self_guided", [True, False])
def test_smooth_sigma_gradients_of_a_volume(self_guided):
    import torch
    K = 2
    image, guide, g = volume_arrays(1)
    with rfa.SmoothPlan.volume(VOLUME_SHAPE[1:], planes=VOLUME_SHAPE[0], guide_planes=0 if self_guided else 1, iterations=K, sigma_s=SIGMA_S,
                               sigma_r=SIGMA_R, spacing_z=2.5, differentiable=True) as plan:
        gd = None if self_guided else cuda(guide)
        ref = [t.clone() for t in plan.backward(cuda(image), gd, cuda(g), edges=True) if t is not None]
        gi, gg, gp = plan.backward_sigmas(cuda(image), gd, cuda(g), edges=True)
        torch.cuda.synchronize()
        assert plan.backward_sigmas_num_kernels(True) == 51 * K - 5
    assert_params(gp.cpu().numpy(), smooth_expected(K, self_guided, "volume"), f"smooth volume self_guided={self_guided}")
    guarded.assert_bits_equal([gi] + ([gg] if gg is not None else []), ref, "volume: grad_image and grad_guide against backward")
    with rfa.SmoothPlan.volume(VOLUME_SHAPE[1:], planes=VOLUME_SHAPE[0], iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R) as unflagged:
        with pytest.raises(rfa.RecFilterError, match="RF_SMOOTH_VOLUME_BACKWARD"):
            unflagged.backward_sigmas(cuda(image), None, cuda(g), edges=False)


def test_smooth_sigma_gradients_with_a_uint8_guide():
    import torch
    K = 2
    image, g = cuda(scases.image(SMOOTH_SHAPE)), cuda(scases.grad_out(SMOOTH_SHAPE))
    with rfa.SmoothPlan(SMOOTH_SHAPE[1:], planes=3, guide_planes=1, guide_dtype=torch.uint8, iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R) as plan:
        guide = cuda(byte_guide())
        ref = plan.backward(image, guide, g, edges=False)[0].clone()
        gi, gg, gp = plan.backward_sigmas(image, guide, g, edges=False)
        with pytest.raises(rfa.RecFilterError, match="uint8 guide"):
            plan.backward_sigmas(image, guide, g, edges=True)
        torch.cuda.synchronize()
    assert gg is None
    assert_params(gp.cpu().numpy(), smooth_expected(K, False, "bytes"), "smooth uint8 guide")
    guarded.assert_bits_equal([gi], [ref], "uint8 guide: grad_image against backward")


def test_smooth_sigma_guarded_planes():
    import torch
    K = 2
    arrays = (scases.image(SMOOTH_SHAPE), scases.guide(SMOOTH_SHAPE, 1), scases.grad_out(SMOOTH_SHAPE))
    roles = []
    for a in arrays:
        views, checker = guarded.guarded_planes(SMOOTH_SHAPE[1:], np.float32, a.shape[0], fill=guarded.IN_FILL)
        checker.load([torch.from_numpy(np.array(p)) for p in a])
        checker.snapshot()
        roles.append((views, checker))
    gi, c_gi = guarded.guarded_planes(SMOOTH_SHAPE[1:], np.float32, 3)
    gg, c_gg = guarded.guarded_planes(SMOOTH_SHAPE[1:], np.float32, 1)
    gp, c_gp = guarded.guarded_planes((3 + K,), np.float64, 1)
    with rfa.SmoothPlan(SMOOTH_SHAPE[1:], planes=3, guide_planes=1, iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R) as plan:
        plan.backward_sigmas(roles[0][0], roles[1][0], roles[2][0], gi, gg, edges=True, grad_params=gp[0])
        torch.cuda.synchronize()
    for checker, what in ((c_gi, "grad_image"), (c_gg, "grad_guide"), (c_gp, "grad_params")):
        checker.check_guards(what)
    for (_, checker), what in zip(roles, ("image", "guide", "grad_out")):
        checker.check_unchanged(what)
    assert_params(gp[0].cpu().numpy(), smooth_expected(K, False), "smooth guarded")


# ---- autograd through the sigmas ----------------------------------------------------------------------------------------------------
def test_edge_aware_smooth_with_tensor_sigmas():
    import torch
    K = 2
    image, g = cuda(scases.image(SMOOTH_SHAPE)), cuda(scases.grad_out(SMOOTH_SHAPE))
    guide = cuda(scases.guide(SMOOTH_SHAPE, 1))
    s = torch.tensor(SIGMA_S, dtype=torch.float64, requires_grad=True)
    r = torch.tensor(SIGMA_R, dtype=torch.float64, requires_grad=True)
    out = rfa.edge_aware_smooth(image, guide, s, r, iterations=K, form="plan", differentiable=True)
    out.backward(g)
    plain = rfa.edge_aware_smooth(image, guide, SIGMA_S, SIGMA_R, iterations=K, form="plan")
    assert guarded.bits_equal(out.detach(), plain)
    assert_params(np.array([s.grad.item(), r.grad.item()]), tuple(v[:2] for v in smooth_expected(K, False)), "edge_aware_smooth tensor sigmas")


def test_edge_aware_smooth_volume_with_tensor_sigmas():
    import torch
    K = 2
    image, _, g = volume_arrays(1)
    s = torch.tensor(SIGMA_S, dtype=torch.float64, requires_grad=True)
    r = torch.tensor(SIGMA_R, dtype=torch.float64, requires_grad=True)
    out = rfa.edge_aware_smooth_volume(cuda(image), None, s, r, iterations=K, spacing_z=2.5, differentiable=True)
    out.backward(cuda(g))
    assert_params(np.array([s.grad.item(), r.grad.item()]), tuple(v[:2] for v in smooth_expected(K, True, "volume")), "edge_aware_smooth_volume tensor sigmas")


def test_two_forwards_then_two_backwards_keep_their_own_sigmas():
    """both calls share one cached plan: the backward of the first must set its sigmas again"""
    import torch
    K = 2
    image, g = cuda(scases.image(SMOOTH_SHAPE)), cuda(scases.grad_out(SMOOTH_SHAPE))
    guide = cuda(scases.guide(SMOOTH_SHAPE, 1))

    def sigmas(vs, vr):
        return torch.tensor(vs, dtype=torch.float64, requires_grad=True), torch.tensor(vr, dtype=torch.float64, requires_grad=True)
    s1, r1 = sigmas(SIGMA_S, SIGMA_R)
    s2, r2 = sigmas(2.0 * SIGMA_S, 0.5 * SIGMA_R)
    out1 = rfa.edge_aware_smooth(image, guide, s1, r1, iterations=K, form="plan", differentiable=True)
    out2 = rfa.edge_aware_smooth(image, guide, s2, r2, iterations=K, form="plan", differentiable=True)
    out1.backward(g)
    out2.backward(g)
    alone = sigmas(2.0 * SIGMA_S, 0.5 * SIGMA_R)
    rfa.edge_aware_smooth(image, guide, *alone, iterations=K, form="plan", differentiable=True).backward(g)
    assert_params(np.array([s1.grad.item(), r1.grad.item()]), tuple(v[:2] for v in smooth_expected(K, False)), "first of two forwards")
    assert s2.grad.item() == alone[0].grad.item() and r2.grad.item() == alone[1].grad.item()
    assert s2.grad.item() != s1.grad.item()
