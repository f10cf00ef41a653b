"""GPU tests of the time-varying direct-form-I section (rf_var2_plan_execute_biquad / _backward_biquad: var2_biquad_tails_1d and
var2_biquad_grad_1d of kernels_var2_signal.hip, plan_var2.cpp, Var2Plan.execute_biquad / biquad_scan of recfilter_amd/var2.py).

Reference: the f64 loops of tests/biquad_loops.py (pinned against scipy.signal.lfilter and central differences in
tests/test_biquad_host.py); cases and bar: tests/biquad_cases.py -- max abs error over the peak <= max(4 x the same figure of the
numpy f32 serial loop, 1e-6), forward and all six gradients.  tests/test_biquad_host.py holds the numpy replay of the kernels under
the same bar on every case here.  Every coefficient the section masks holds NaN; inputs are seeded, signed, in [-1, 1].

The long case, 4,198,404 samples, is 1026 groups: var2_carry_1d takes two sweeps.  It is of the sprinkled family and is checked
against the segmented loops."""
import os
import subprocess
import sys

import numpy as np
import pytest

import biquad_cases as cases
import biquad_emulator as emu
import guarded
import var2_exact as exact
import recfilter_amd as rfa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = [True, False]
GRADS = cases.NAMES[1:]


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


def host(t, lines):
    return t.cpu().numpy().reshape(lines, -1)


def run_forward(plan, inputs, stride=None):
    """execute_biquad on host arrays (x, b0, b1, b2, a1, a2); the result on the host"""
    import torch
    out = plan.execute_biquad(*(device_lines(a, stride) for a in inputs))
    torch.cuda.synchronize()
    return host(out, np.asarray(inputs[0]).shape[0])


def run_backward(plan, inputs, y, g, with_coefficients, stride=None):
    """[grad_x, grad_b0, ..., grad_a2] on the host (grad_x alone without coefficient gradients); what the call writes is NaN before"""
    import torch
    shape = np.asarray(g).shape
    d = [device_lines(a, stride) for a in inputs]
    grads = None
    if with_coefficients:
        grads = tuple(device_lines(np.full(shape, np.nan, np.float32), stride) for _ in range(5))
    gin, grads = plan.backward_biquad(*d, device_lines(y, stride) if with_coefficients else None, device_lines(g, stride), None, grads)
    torch.cuda.synchronize()
    return [host(t, shape[0]) for t in (gin,) + (grads or ())]


def assert_masked_gradients_are_zero(full, causal, what):
    one, two = (np.s_[:, :1], np.s_[:, :2]) if causal else (np.s_[:, -1:], np.s_[:, -2:])
    gb1, gb2, ga1, ga2 = full[2:6]
    for grad, where in ((gb1, one), (gb2, two), (ga1, one), (ga2, two)):
        assert np.all(bits(grad[where]) == 0), f"{what}: the masked coefficients' gradients are not +0"


def check_all(n, lines, kind, causal, stride=None):
    """the forward and the backward without and with coefficient gradients of one case under the bar"""
    signals = cases.case(n, lines, kind, causal)
    inputs, g = signals[:6], signals[6]
    want = cases.expected(n, lines, kind, causal)
    what = f"{n} x {lines} {kind} {name_of(causal)}"
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        y = run_forward(plan, inputs, stride)
        cases.assert_under_bar(y, want["out"], f"{what} out")
        only_x = run_backward(plan, inputs, y, g, False, stride)
        full = run_backward(plan, inputs, y, g, True, stride)
    assert len(only_x) == 1 and len(full) == 6
    np.testing.assert_array_equal(bits(only_x[0]), bits(full[0]))      # with or without the coefficient gradients
    # (the reference's gradients take the f64 forward as y; the kernels' take their own f32 forward, as a caller's do)
    for got, name in zip(full, GRADS):
        cases.assert_under_bar(got, want[name], f"{what} {name}")
    assert_masked_gradients_are_zero(full, causal, what)


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("n", cases.LENGTHS)
def test_against_f64_loops(n, kind, causal):
    check_all(n, 1, kind, causal)


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("lines,n,stride", cases.LINE_CASES)
def test_lines_with_a_stride_above_the_length(lines, n, stride, causal):
    check_all(n, lines, "resonator", causal, stride)


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_long_signal_against_segmented_loops(causal):
    check_all(cases.LONG, 1, "sprinkled", causal)


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n,lines,kind", cases.LONG_MEMORY_CASES)
def test_long_memory_against_f64_loops(n, lines, kind, causal):
    """r inside [0.998, 0.9995] at four groups: a group's P reaches the result (tests/var2_cases.py); the seeds are the ones under
    which the numpy replay is at or below half the bar (cases.LONG_MEMORY_SEEDS)"""
    assert cases.LONG_MEMORY_CASES == [(12292, 1, "long memory")]      # the ones tests/test_biquad_host.py holds the replay on
    check_all(n, lines, kind, causal)


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("family", list(exact.FAMILIES))
@pytest.mark.parametrize("n", exact.LENGTHS[:2])
def test_integer_rotations_with_integer_taps_are_exact(n, family, causal):
    """tests/var2_exact.py: constant integer taps in front of a companion matrix of period 6 or 3 or the running sum's, inputs in
    {-1, 0, 1} -- the output and all six gradients are the integers, bit for bit, at four groups and at 66"""
    signals = exact.biquad_case(n, family, causal)
    want = exact.biquad_expected(n, family, causal)
    what = f"{n} {family} {name_of(causal)}"
    with rfa.Var2Plan(n, causal=causal) as plan:
        y = run_forward(plan, signals[:6])
        exact.assert_equal(y, want["out"], f"{what} out", causal)
        only_x = run_backward(plan, signals[:6], y, signals[6], False)
        full = run_backward(plan, signals[:6], y, signals[6], True)
    np.testing.assert_array_equal(bits(only_x[0]), bits(full[0]))
    for got, name in zip(full, GRADS):
        exact.assert_equal(got, want[name], f"{what} {name}", causal)
    assert_masked_gradients_are_zero(full, causal, what)


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [68, 8196])
def test_unit_taps_give_the_bits_of_the_all_pole_scan(n, causal):
    import torch
    x, _, _, _, a1, a2, _ = cases.case(n, 1, "resonator", causal)
    one, zero = np.ones_like(x), np.zeros_like(x)
    with rfa.Var2Plan(n, causal=causal) as plan:
        got = run_forward(plan, (x, one, zero, zero, a1, a2))
        want = plan.execute(*(device_lines(a) for a in (x, a1, a2)))
        torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(got), bits(host(want, 1)))


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [68, 8196, cases.LONG])
def test_zero_feedback_gives_the_bits_of_the_emulators_feed_forward_part(n, causal):
    x, b0, b1, b2, _, _, _ = cases.case(n, 1, "sprinkled" if n == cases.LONG else "resonator", causal)
    zero = np.zeros_like(x)
    with rfa.Var2Plan(n, causal=causal) as plan:
        got = run_forward(plan, (x, b0, b1, b2, zero, zero))
    np.testing.assert_array_equal(bits(got[0]), bits(emu.feed_forward(x[0], b0[0], b1[0], b2[0], causal)))


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_a_nan_in_every_masked_slot_changes_nothing(causal):
    n = 4100
    signals = cases.case(n, 1, "resonator", causal)
    inputs, g = signals[:6], signals[6]
    assert [int(np.isnan(s).sum()) for s in inputs] == [0, 0, 1, 2, 1, 2]
    cleared = tuple(np.nan_to_num(s, nan=0.0) for s in inputs)
    with rfa.Var2Plan(n, causal=causal) as plan:
        y = run_forward(plan, inputs)
        np.testing.assert_array_equal(bits(y), bits(run_forward(plan, cleared)))
        full = run_backward(plan, inputs, y, g, True)
        for a, b in zip(full, run_backward(plan, cleared, y, g, True)):
            assert not np.isnan(a).any()
            np.testing.assert_array_equal(bits(a), bits(b))
    assert_masked_gradients_are_zero(full, causal, f"NaN in the masked slots, {name_of(causal)}")


# ---- state, guards ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
def test_runs_agree_and_a_plan_keeps_no_state(causal):
    import torch
    n = 8196
    signals = cases.case(n, 1, "near one", causal)
    inputs, g = signals[:6], signals[6]
    with rfa.Var2Plan(n, causal=causal) as other:
        fresh = run_forward(other, inputs)
    with rfa.Var2Plan(n, causal=causal) as plan:
        d = [device_lines(v) for v in inputs]
        poison = torch.full_like(d[0], float("nan"))
        results = [plan.execute_biquad(*d)]
        plan.execute_biquad(poison, *d[1:])      # a NaN input in between
        results += [plan.execute_biquad(*d) for _ in range(2)]
        torch.cuda.synchronize()
        for r in results[1:]:
            guarded.assert_bits_equal([r.cpu()], [results[0].cpu()], "repeated executes of one plan")
        np.testing.assert_array_equal(bits(host(results[0], 1)), bits(fresh))
        first = run_backward(plan, inputs, fresh, g, True)
        plan.execute_biquad(poison, *d[1:])
        plan.backward_biquad(*d, None, poison)      # and a NaN gradient through the plan's adjoint-state signal
        for a, b in zip(first, run_backward(plan, inputs, fresh, g, True)):
            np.testing.assert_array_equal(bits(a), bits(b))


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [4100, 8196])
def test_guarded_signals(n, causal):
    """the input, the five coefficients and grad_out, the output and the six gradients between guards: nothing outside them is
    read (the guards of what is read hold NaN) or written"""
    import torch
    signals = cases.case(n, 1, "resonator", causal)
    want = cases.expected(n, 1, "resonator", causal)
    read, g_read = guarded.guarded_planes((n,), np.float32, 7, fill=guarded.IN_FILL)
    written, g_written = guarded.guarded_planes((n,), np.float32, 7, fill=guarded.OUT_FILL)
    g_read.load([torch.from_numpy(np.array(a[0])) for a in signals])
    g_read.snapshot()
    with rfa.Var2Plan(n, causal=causal) as plan:
        plan.execute_biquad(*read[:6], written[0])
        plan.backward_biquad(*read[:6], written[0], read[6], written[1], tuple(written[2:]))
        torch.cuda.synchronize()
    g_written.check_guards("output and gradients")
    g_read.check_unchanged("input, coefficients and grad_out")
    for t, name in zip(written, cases.NAMES):
        cases.assert_under_bar(host(t, 1), want[name], f"guarded {n} {name_of(causal)} {name}")


# ---- front-ends -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("lines,n", [(1, 5), (2, 4101)])
def test_biquad_scan_and_its_gradients(lines, n, causal):
    """biquad_scan(...).backward() against the f64 loops on the unpadded signals: 5 is padded to 8 and 4101 to 4104 -- behind the end
    (causal) or before the start (anticausal) -- and sliced back"""
    import torch
    rng = np.random.default_rng(100 * n + lines)
    shape = (lines, n)
    x, g = ((rng.random(shape) * 2 - 1).astype(np.float32) for _ in range(2))
    a1, a2 = cases.var2_cases.coefficients("resonator", shape, rng)
    signals = (x, *cases.taps(shape, rng), a1, a2, g)
    want = cases.reference(signals, causal)
    squeeze = (lambda a: a[0]) if lines == 1 else (lambda a: a)
    d = [torch.from_numpy(squeeze(a)).cuda().requires_grad_() for a in signals[:6]]
    out = rfa.biquad_scan(*d, causal=causal)
    assert tuple(out.shape) == tuple(d[0].shape)
    out.backward(torch.from_numpy(squeeze(g)).cuda())
    torch.cuda.synchronize()
    for t, name in zip([out.detach()] + [t.grad for t in d], cases.NAMES):
        cases.assert_under_bar(host(t, lines), want[name], f"biquad_scan {lines} x {n} {name_of(causal)} {name}")
    # the input's gradient alone: the same bits
    x2 = torch.from_numpy(squeeze(x)).cuda().requires_grad_()
    rfa.biquad_scan(x2, *(t.detach() for t in d[1:]), causal=causal).backward(torch.from_numpy(squeeze(g)).cuda())
    np.testing.assert_array_equal(bits(x2.grad.cpu().numpy()), bits(d[0].grad.cpu().numpy()))


def test_launch_names_and_call_refusals():
    import torch
    n = 4100
    x = torch.zeros(n, device="cuda")
    b = [torch.full((n,), v, device="cuda") for v in (1.0, -0.5, 0.25)]
    a = [torch.full((n,), v, device="cuda") for v in (-0.5, 0.25)]
    new = lambda: torch.empty_like(x)
    with rfa.Var2Plan(n) as plan:
        assert plan.backward_biquad_bytes == 4 * n
        y, times = plan.execute_biquad_timed(x, *b, *a)
        assert [name for name, _ in times] == ["var2_biquad_tails_1d", "var2_carry_1d", "var2_pass2_1d"]
        assert all(ms >= 0 for _, ms in times)
        backward = ["var2_adj_tails_1d", "var2_carry_1d", "var2_adj_pass2_1d", "var2_biquad_grad_1d"]
        *_, times = plan.backward_biquad_timed(x, *b, *a, None, x)
        assert [name for name, _ in times] == backward
        *_, times = plan.backward_biquad_timed(x, *b, *a, y, x, None, tuple(new() for _ in range(5)))
        assert [name for name, _ in times] == backward
        g = torch.ones(n, device="cuda")
        gin, _ = plan.backward_biquad(x, *b, *a, None, g, g)      # grad_in == grad_out is allowed
        assert gin.data_ptr() == g.data_ptr()
        refused = [
            lambda: plan.execute_biquad(x, *b, *a, x),                                           # in == out
            lambda: plan.execute_biquad(x, *b, *a, b[1]),                                        # a coefficient signal that is the output
            lambda: plan.execute_biquad(torch.zeros(n + 4, device="cuda")[1:1 + n], *b, *a),     # 4 bytes off a 16-byte boundary
            lambda: plan.backward_biquad(x, *b, *a, y, g, None, (new(), new(), None, new(), new())),      # a mix
            lambda: plan.backward_biquad(x, *b, *a, None, g, None, tuple(new() for _ in range(5))),       # coefficient gradients need out
            lambda: plan.backward_biquad(x, *b, *a, y, g, x),                                    # a gradient written over what is read
        ]
        for i, call in enumerate(refused):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG, i
            assert len(str(e.value)) > 30, i
        torch.cuda.synchronize()


def test_cpp_frontend_biquad(tmp_path):
    """RecFilterVarying2::realize_biquad / gradient_biquad on a signal of 12356 samples, both directions, against loops in the C++
    file; compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_biquad.cpp")
    exe = str(tmp_path / "test_frontend_biquad")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "biquad-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
