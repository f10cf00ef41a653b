"""GPU tests of the cascade for training (rf_var2_plan_execute_cascade_keep / _backward_cascade_kept: var2_adj_link_1d,
var2_adj_link_keep_1d and var2_biquad_coef_1d of kernels_var2_signal.hip, plan_var2.cpp, Var2Plan.execute_cascade_keep /
backward_cascade_kept / biquad_cascade(keep=True) of recfilter_amd/var2.py).

Reference, cases and bar are those of tests/test_gpu_cascade_signal.py: the f64 loops of tests/cascade_loops.py, the cases of
tests/cascade_cases.py, max abs error over the peak <= max(4 x the same figure of the numpy f32 serial cascade, 1e-6) on grad_x
and all 5 K coefficient gradients.  tests/test_cascade_kept_host.py holds the numpy replay of the new backward to half that bar
on every case here (all but the 4,198,404-sample line, whose carry stage is unchanged).

The exact identities pin the adjoint link: with all feedback coefficients 0 the stored maps reproduce the samples exactly, the
state that enters a tile in the adjoint scan IS the neighbouring tile's lam, and backward_cascade_kept is backward_cascade bit
for bit.  With feedback the two differ in the last bits of a few samples: no equality is asserted there."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cascade_cases as cases
import guarded
import var2_exact as exact
import recfilter_amd as rfa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = cases.DIRECTIONS


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def name_of(causal):
    return "causal" if causal else "anticausal"


def device_lines(a, stride=None):
    """an (L, N) array on the device: (N,) for one line, else rows `stride` apart (NaN between them)"""
    import torch
    a = np.asarray(a)
    lines, n = a.shape
    if lines == 1:
        return torch.from_numpy(np.array(a[0])).cuda()
    wide = torch.full((lines, stride or n), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :n] = torch.from_numpy(np.array(a)).cuda()
    return wide[:, :n]


def device_sections(sections, stride=None):
    return [tuple(device_lines(c, stride) for c in s) for s in sections]


def host(t, lines):
    return t.cpu().numpy().reshape(lines, -1)


def nan_lines(shape, stride=None):
    return device_lines(np.full(shape, np.nan, np.float32), stride)


def keep_forward(plan, x, sections, stride=None):
    """(dx, ds, out, kept) on the device; what the call writes is NaN before"""
    import torch
    shape = np.asarray(x).shape
    dx, ds = device_lines(x, stride), device_sections(sections, stride)
    out, kept = plan.execute_cascade_keep(dx, ds, nan_lines(shape, stride), [nan_lines(shape, stride) for _ in sections[1:]])
    torch.cuda.synchronize()
    assert len(kept) == len(sections) - 1
    return dx, ds, out, kept


def kept_backward(plan, forward, g, with_coefficients, stride=None, backward=None):
    """[grad_x, then the 5 K coefficient gradients] on the host (grad_x alone without them, and then NOTHING of the forward is
    handed in); what the call writes is NaN before"""
    import torch
    dx, ds, out, kept = forward
    shape = np.asarray(g).shape
    grads = [tuple(nan_lines(shape, stride) for _ in range(5)) for _ in ds] if with_coefficients else None
    dg = device_lines(g, stride)
    if with_coefficients:
        gin, grads = (backward or plan.backward_cascade_kept)(dx, ds, kept, out, dg, nan_lines(shape, stride), grads)
    else:
        gin, grads = (backward or plan.backward_cascade_kept)(None, ds, None, None, dg, nan_lines(shape, stride), None)
    torch.cuda.synchronize()
    return [host(t, shape[0]) for t in [gin] + [t for s in (grads or ()) for t in s]]


def old_backward(plan, forward, g, stride=None):
    import torch
    dx, ds, out, _ = forward
    shape = np.asarray(g).shape
    grads = [tuple(nan_lines(shape, stride) for _ in range(5)) for _ in ds]
    gin, grads = plan.backward_cascade(dx, ds, out, device_lines(g, stride), None, grads)
    torch.cuda.synchronize()
    return [host(t, shape[0]) for t in [gin] + [t for s in grads for t in s]]


def assert_masked_gradients_are_zero(full, causal, K, what):
    one, two = (np.s_[:, :1], np.s_[:, :2]) if causal else (np.s_[:, -1:], np.s_[:, -2:])
    for k in range(K):
        gb1, gb2, ga1, ga2 = full[1 + 5 * k + 1], full[1 + 5 * k + 2], full[1 + 5 * k + 3], full[1 + 5 * k + 4]
        for grad, where in ((gb1, one), (gb2, two), (ga1, one), (ga2, two)):
            assert np.all(bits(grad[where]) == 0), f"{what}: the masked coefficients' gradients of section {k} are not +0"


def check_all(n, lines, kind, causal, K, stride=None):
    """execute_cascade_keep, then backward_cascade_kept without and with coefficient gradients, of one case under the bar"""
    x, sections, g = cases.case(n, lines, kind, causal, K)
    want = cases.expected(n, lines, kind, causal, K)
    what = f"kept {n} x {lines} {kind} K={K} {name_of(causal)}"
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        forward = keep_forward(plan, x, sections, stride)
        cases.assert_under_bar(host(forward[2], lines), want["out"], f"{what} out")
        only_x = kept_backward(plan, forward, g, False, stride)
        full = kept_backward(plan, forward, g, True, stride)
    assert len(only_x) == 1 and len(full) == 1 + 5 * K
    np.testing.assert_array_equal(bits(only_x[0]), bits(full[0]))      # with or without the coefficient gradients
    worst = max(cases.assert_under_bar(got, want[name], f"{what} {name}") for got, name in zip(full, cases.names(K)[1:]))
    assert_masked_gradients_are_zero(full, causal, K, what)
    print(f"{what}: worst ratio to the f32 serial cascade {worst:.2f}")


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("n", cases.LENGTHS)
@pytest.mark.parametrize("K", [1, 2, 4])
def test_against_f64_loops(K, n, kind, causal):
    check_all(n, 1, kind, causal, K)


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("kind", ["resonator", "sprinkled"])
@pytest.mark.parametrize("n", [4100, 8196])
def test_eight_sections_against_f64_loops(n, kind, causal):
    check_all(n, 1, kind, causal, 8)


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("lines,n,stride", cases.LINE_CASES)
def test_lines_with_a_stride_above_the_length(lines, n, stride, causal):
    check_all(n, lines, "resonator", causal, 2, stride)


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_long_memory_against_f64_loops(causal):
    """r inside [0.998, 0.9995] at four groups, K = 2: a group's P reaches the gradients through var2_adj_link_1d"""
    assert cases.LONG_MEMORY_CASES == [(12292, 1, "long memory", 2)]
    check_all(12292, 1, "long memory", causal, 2)


# ---- exact ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
def test_integer_rotations_of_two_periods_are_exact(causal):
    """tests/var2_exact.py at four groups: a section of period 6 into one of period 3, integer taps, inputs in {-1, 0, 1}.  The
    state that enters every tile of the adjoint link is an integer that never decayed -- a carry that matters -- and the output
    and all 11 gradients are the integers, no tolerance"""
    n = 12292
    assert n == exact.LENGTHS[0]
    x, sections, g = exact.cascade_case(n, causal)
    want, left_out = exact.cascade_expected(n, causal)
    assert not left_out, f"gradients that reach 2^24 and could not be compared: {left_out}"
    what = f"kept {n} period 6 into period 3 {name_of(causal)}"
    with rfa.Var2Plan(n, causal=causal) as plan:
        forward = keep_forward(plan, x, sections)
        exact.assert_equal(host(forward[2], 1), want["out"], f"{what} out", causal)
        only_x = kept_backward(plan, forward, g, False)
        full = kept_backward(plan, forward, g, True)
    np.testing.assert_array_equal(bits(only_x[0]), bits(full[0]))
    for got, name in zip(full, cases.names(2)[1:]):
        exact.assert_equal(got, want[name], f"{what} {name}", causal)
    assert_masked_gradients_are_zero(full, causal, 2, what)


# ---- identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [68, 4100, 8196])
def test_out_and_kept_signals_are_execute_cascades_bits(n, causal):
    """out is execute_cascade's, kept[k] is execute_cascade on sections[:k + 1]"""
    import torch
    K = 4
    x, sections, _ = cases.case(n, 1, "resonator", causal, K)
    with rfa.Var2Plan(n, causal=causal) as plan:
        dx, ds, out, kept = keep_forward(plan, x, sections)
        for k in range(K):
            want = plan.execute_cascade(dx, ds[:k + 1])
            torch.cuda.synchronize()
            got = out if k == K - 1 else kept[k]
            np.testing.assert_array_equal(bits(host(got, 1)), bits(host(want, 1)), f"section {k}")


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [64, 68, 4096, 4100, 8196])
def test_zero_feedback_is_backward_cascade_in_bits(n, causal):
    """all a = 0: all 1 + 5 K outputs of backward_cascade_kept are backward_cascade's bit for bit -- the adjoint link's neighbour
    indexing at tile and group edges"""
    K = 4
    x, sections, g = cases.case(n, 1, "resonator", causal, K)
    zero = np.zeros_like(x)
    sections = tuple((b0, b1, b2, zero, zero) for b0, b1, b2, _, _ in sections)
    with rfa.Var2Plan(n, causal=causal) as plan:
        forward = keep_forward(plan, x, sections)
        got = kept_backward(plan, forward, g, True)
        want = old_backward(plan, forward, g)
    assert len(got) == len(want) == 1 + 5 * K
    for a, b, name in zip(got, want, cases.names(K)[1:]):
        assert not np.isnan(a).any(), name
        np.testing.assert_array_equal(bits(a), bits(b), name)


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [68, 8196])
def test_one_section_is_backward_biquad(n, causal):
    """K = 1, kept null: backward_biquad's launches and bits"""
    import torch
    x, sections, g = cases.case(n, 1, "resonator", causal, 1)
    with rfa.Var2Plan(n, causal=causal) as plan:
        dx, ds, out, kept = keep_forward(plan, x, sections)
        assert kept == []
        want_out = plan.execute_biquad(dx, *ds[0])
        want = plan.backward_biquad(dx, *ds[0], out, device_lines(g), nan_lines(x.shape), tuple(nan_lines(x.shape) for _ in range(5)))
        torch.cuda.synchronize()
        want = [host(t, 1) for t in (want[0], *want[1])]
        np.testing.assert_array_equal(bits(host(out, 1)), bits(host(want_out, 1)))
        full = kept_backward(plan, (dx, ds, out, None), g, True)      # kept: a null pointer
        only_x = kept_backward(plan, (dx, ds, out, None), g, False)
    np.testing.assert_array_equal(bits(only_x[0]), bits(want[0]))
    assert len(full) == len(want) == 6
    for a, b in zip(full, want):
        np.testing.assert_array_equal(bits(a), bits(b))


# ---- state, guards ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
def test_old_and_new_backwards_mix_on_one_plan(causal):
    """kept at K = 4, kept at K = 2, the rerunning backward at K = 4 (it regrows the plan's signals), a NaN grad_out through the
    kept backward, kept at K = 4 again: the first and the last agree in bits, and with a fresh plan's"""
    import torch
    n, K = 8196, 4
    x, sections, g = cases.case(n, 1, "near one", causal, K)
    with rfa.Var2Plan(n, causal=causal) as other:
        fresh = kept_backward(other, keep_forward(other, x, sections), g, True)
    with rfa.Var2Plan(n, causal=causal) as plan:
        forward = keep_forward(plan, x, sections)
        first = kept_backward(plan, forward, g, True)
        assert plan.backward_cascade_kept_bytes(4) == 2 * 4 * n and plan.backward_cascade_bytes(4) == 5 * 4 * n
        kept_backward(plan, keep_forward(plan, x, sections[:2]), g, True)
        old = old_backward(plan, forward, g)
        kept_backward(plan, forward, np.full_like(g, np.nan), True)
        last = kept_backward(plan, forward, g, True)
        torch.cuda.synchronize()
    want = cases.expected(n, 1, "near one", causal, K)
    for a, b, c, o, name in zip(first, last, fresh, old, cases.names(K)[1:]):
        np.testing.assert_array_equal(bits(a), bits(b), name)
        np.testing.assert_array_equal(bits(a), bits(c), name)
        cases.assert_under_bar(o, want[name], f"the rerunning backward between kept ones, {name_of(causal)} {name}")
    # the other order: the rerunning backward first on a new plan, then the kept one on its allocation
    with rfa.Var2Plan(n, causal=causal) as plan:
        forward = keep_forward(plan, x, sections)
        old_backward(plan, forward, g)
        for a, b, name in zip(first, kept_backward(plan, forward, g, True), cases.names(K)[1:]):
            np.testing.assert_array_equal(bits(a), bits(b), name)


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [68, 4100])
def test_guarded_signals(n, causal):
    """the input, the ten coefficients and grad_out, the output, the kept signal and the eleven gradients between guards: nothing
    outside them is read (the guards of what is read hold NaN) or written"""
    import torch
    K = 2
    x, sections, g = cases.case(n, 1, "resonator", causal, K)
    want = cases.expected(n, 1, "resonator", causal, K)
    read, g_read = guarded.guarded_planes((n,), np.float32, 2 + 5 * K, fill=guarded.IN_FILL)
    written, g_written = guarded.guarded_planes((n,), np.float32, 3 + 5 * K, fill=guarded.OUT_FILL)
    g_read.load([torch.from_numpy(np.array(a[0])) for a in (x, g, *(c for s in sections for c in s))])
    g_read.snapshot()
    ds = [tuple(read[2 + 5 * k:7 + 5 * k]) for k in range(K)]
    grads = [tuple(written[2 + 5 * k:7 + 5 * k]) for k in range(K)]
    kept = [written[2 + 5 * K]]
    with rfa.Var2Plan(n, causal=causal) as plan:
        plan.execute_cascade_keep(read[0], ds, written[0], kept)
        plan.backward_cascade_kept(read[0], ds, kept, written[0], read[1], written[1], grads)
        torch.cuda.synchronize()
        first = plan.execute_cascade(read[0], ds[:1])
        torch.cuda.synchronize()
    g_written.check_guards("output, kept signal and gradients")
    g_read.check_unchanged("input, coefficients and grad_out")
    np.testing.assert_array_equal(bits(host(kept[0], 1)), bits(host(first, 1)))
    for t, name in zip(written, cases.names(K)):
        cases.assert_under_bar(host(t, 1), want[name], f"guarded kept {n} {name_of(causal)} {name}")


# ---- launches ---------------------------------------------------------------------------------------------------------------------
def test_launch_names_counts_and_call_refusals():
    import torch
    n = 4100
    x = torch.zeros(n, device="cuda")
    new = lambda: torch.empty_like(x)      # noqa: E731
    section = tuple(torch.full((n,), v, device="cuda") for v in (1.0, -0.5, 0.25, -0.5, 0.25))
    with rfa.Var2Plan(n) as plan:
        for K in (1, 2, 3, 16):
            sections = [section] * K
            y, kept, times = plan.execute_cascade_keep_timed(x, sections)
            want = ["var2_biquad_tails_1d"] + ["var2_carry_1d", "var2_link_keep_1d"] * (K - 1) + ["var2_carry_1d", "var2_pass2_1d"]
            assert [name for name, _ in times] == want and len(want) == 2 * K + 1 == plan.cascade_num_kernels(K)
            assert all(ms >= 0 for _, ms in times) and len(kept) == K - 1
            last = ["var2_carry_1d", "var2_adj_pass2_1d", "var2_biquad_grad_1d"]
            want = ["var2_adj_tails_1d"] + ["var2_carry_1d", "var2_adj_link_1d"] * (K - 1) + last
            assert len(want) == 2 * K + 2 == plan.backward_cascade_kept_num_kernels(K, False)
            *_, times = plan.backward_cascade_kept_timed(None, sections, None, None, x)
            assert [name for name, _ in times] == want
            want = ["var2_adj_tails_1d"] + ["var2_carry_1d", "var2_adj_link_keep_1d", "var2_biquad_coef_1d"] * (K - 1) + last
            assert len(want) == 3 * K + 1 == plan.backward_cascade_kept_num_kernels(K, True)
            *_, times = plan.backward_cascade_kept_timed(x, sections, kept, y, x, None, [tuple(new() for _ in range(5)) for _ in range(K)])
            assert [name for name, _ in times] == want
        g = torch.ones(n, device="cuda")
        two = [section, section]
        y, kept = plan.execute_cascade_keep(x, two)
        gin, _ = plan.backward_cascade_kept(x, two, kept, y, g, g, [tuple(new() for _ in range(5)) for _ in range(2)])      # grad_in == grad_out
        assert gin.data_ptr() == g.data_ptr()
        five = lambda: [tuple(new() for _ in range(5)) for _ in range(2)]      # noqa: E731
        refused = [
            lambda: plan.execute_cascade_keep(x, two, x),                                        # in == out
            lambda: plan.execute_cascade_keep(x, two, None, [x]),                                # a kept signal that is the input
            lambda: plan.execute_cascade_keep(x, two, y, [y]),                                   # a kept signal that is the output
            lambda: plan.execute_cascade_keep(x, two, None, [section[3]]),                       # a kept signal that is a coefficient
            lambda: plan.execute_cascade_keep(x, []),                                            # no section
            lambda: plan.backward_cascade_kept(x, two, None, y, g, None, five()),                # gradients need the kept signals
            lambda: plan.backward_cascade_kept(x, two, kept, None, g, None, five()),             # and out
            lambda: plan.backward_cascade_kept(None, two, kept, y, g, None, five()),             # and in
            lambda: plan.backward_cascade_kept(x, two, kept, y, g, kept[0], five()),             # a gradient written over a kept signal
            lambda: plan.backward_cascade_kept(x, two, kept, y, g, None, [tuple(new() for _ in range(5)), (new(), new(), None, new(), new())]),
        ]
        for i, call in enumerate(refused):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG, i
            assert len(str(e.value)) > 15, i
        torch.cuda.synchronize()


# ---- front-ends -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("lines,n", [(1, 5), (2, 4101)])
def test_biquad_cascade_keep_and_its_gradients(lines, n, causal):
    """biquad_cascade(..., keep=True).backward() against the f64 loops on the unpadded signals (5 is padded to 8, 4101 to 4104);
    keep=True with x alone requiring a gradient gives grad_x's bits; keep=False gives the rerunning route's bits"""
    import torch
    import cascade_loops as loops
    K = 3
    rng = np.random.default_rng(300 * n + lines)
    shape = (lines, n)
    x, g = ((rng.random(shape) * 2 - 1).astype(np.float32) for _ in range(2))
    sections = []
    for _ in range(K):
        a1, a2 = cases.var2_cases.coefficients("resonator", shape, rng)
        sections.append((*cases.biquad_cases.taps(shape, rng), a1, a2))
    results = {}
    for dtype in (np.float64, np.float32):
        ys = loops.forward(x, sections, causal, dtype)
        results[dtype] = cases.flat(ys[-1], loops.adjoint(x, sections, ys, g, causal, dtype))
    want = {}
    for name, ref, serial in zip(cases.names(K), results[np.float64], results[np.float32]):
        peak = max(float(np.max(np.abs(ref))), 1e-30)
        want[name] = (ref, cases._figure(serial, ref, peak), peak)
    squeeze = (lambda a: a[0]) if lines == 1 else (lambda a: a)

    def leaves():
        return (torch.from_numpy(squeeze(x)).cuda().requires_grad_(),
                [tuple(torch.from_numpy(squeeze(c)).cuda().requires_grad_() for c in s) for s in sections])
    dg = torch.from_numpy(squeeze(g)).cuda()
    dx, ds = leaves()
    out = rfa.biquad_cascade(dx, ds, causal=causal, keep=True)
    assert tuple(out.shape) == tuple(dx.shape)
    out.backward(dg)
    torch.cuda.synchronize()
    kept_route = [out.detach(), dx.grad] + [c.grad for s in ds for c in s]
    for a, name in zip(kept_route, cases.names(K)):
        cases.assert_under_bar(host(a, lines), want[name], f"biquad_cascade keep=True {lines} x {n} {name_of(causal)} {name}")
    # the input's gradient alone: the plain forward, nothing saved but the coefficients, the same bits
    x2 = torch.from_numpy(squeeze(x)).cuda().requires_grad_()
    out2 = rfa.biquad_cascade(x2, [tuple(c.detach() for c in s) for s in ds], causal=causal, keep=True)
    out2.backward(dg)
    np.testing.assert_array_equal(bits(out2.detach().cpu().numpy()), bits(out.detach().cpu().numpy()))
    np.testing.assert_array_equal(bits(x2.grad.cpu().numpy()), bits(dx.grad.cpu().numpy()))
    # keep=False: the default's bits, forward and all gradients
    ex, es = leaves()
    default = rfa.biquad_cascade(ex, es, causal=causal)
    default.backward(dg)
    fx, fs = leaves()
    explicit = rfa.biquad_cascade(fx, fs, causal=causal, keep=False)
    explicit.backward(dg)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(default.detach().cpu().numpy()), bits(out.detach().cpu().numpy()))
    for a, b in zip([explicit.detach(), fx.grad] + [c.grad for s in fs for c in s], [default.detach(), ex.grad] + [c.grad for s in es for c in s]):
        np.testing.assert_array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))


def test_cpp_frontend_cascade_kept(tmp_path):
    """RecFilterVarying2::realize_cascade_keep / gradient_cascade_kept on a signal of 12356 samples, both directions, against
    loops in the C++ file; compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_cascade_kept.cpp")
    exe = str(tmp_path / "test_frontend_cascade_kept")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "cascade-kept-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
