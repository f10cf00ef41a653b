"""GPU tests of the time-varying second-order all-pole scans (rf_var2_plan_*: kernels_var2_signal.hip, plan_var2.cpp, Var2Plan /
allpole_scan of recfilter_amd/var2.py).

Reference: the f64 loops of tests/var2_loops.py (pinned by central differences in tests/test_var2_host.py); cases and bar:
tests/var2_cases.py -- max abs error over the peak <= max(4 x the same figure of the numpy f32 serial loop, 1e-6), forward and
gradients.  tests/test_var2_host.py holds the numpy replay of the kernels' algebra under the same bar on every case here.  The
coefficients a scan masks hold NaN; inputs are seeded, signed, in [-1, 1].

The long case, 4,198,404 samples, is 1026 groups: var2_carry_1d takes two sweeps.  It is of the sprinkled family, whose zeros cut
the line every 200..600 samples, and is checked against the segmented loops.

With a pole radius of at most 0.98 a group's 2 x 2 matrix P is 0.98^4096 = 1e-36: those families cannot see the matrix half of
var2_carry_1d.  Two families can: the integer rotations of tests/var2_exact.py, compared without tolerance, and the long-memory
family (r inside [0.998, 0.9995]) under the bar; tests/test_var2_carry_seen_host.py shows on the CPU that a wrong carry stage
fails every one of their cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guarded
import var2_cases as cases
import var2_exact as exact
import recfilter_amd as rfa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = [True, False]


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


def run_forward(n, lines, causal, x, a1, a2, stride=None, inplace=False):
    import torch
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        dx = device_lines(x, stride)
        out = plan.execute(dx, device_lines(a1, stride), device_lines(a2, stride), dx if inplace else None)
        torch.cuda.synchronize()
        return host(out, lines)


def run_backward(plan, a1, a2, y, g, with_coefficients, stride=None):
    """(grad_x, grad_a1, grad_a2) on the host; the gradients the call writes are NaN before it"""
    import torch
    lines = np.asarray(g).shape[0]
    d1, d2, dy, dg = (device_lines(a, stride) for a in (a1, a2, y, g))
    g1 = g2 = None
    if with_coefficients:
        g1, g2 = (device_lines(np.full(np.asarray(g).shape, np.nan, np.float32), stride) for _ in range(2))
    gin, g1, g2 = plan.backward(d1, d2, dy if with_coefficients else None, dg, None, g1, g2)
    torch.cuda.synchronize()
    return tuple(None if t is None else host(t, lines) for t in (gin, g1, g2))


def check_all(n, lines, kind, causal, stride=None):
    """the forward and the backward with and without coefficient gradients of one case under the bar; returns the worst ratios"""
    x, a1, a2, g = cases.case(n, lines, kind, causal)
    want = cases.expected(n, lines, kind, causal)
    what = f"{n} x {lines} {kind} {name_of(causal)}"
    y = run_forward(n, lines, causal, x, a1, a2, stride)
    forward = cases.assert_under_bar(y, want["out"], f"{what} out")
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        only_x = run_backward(plan, a1, a2, y, g, False, stride)
        full = run_backward(plan, a1, a2, y, g, True, stride)
    assert only_x[1] is None and only_x[2] is None
    np.testing.assert_array_equal(bits(only_x[0]), bits(full[0]))      # with or without the coefficient gradients
    # (the reference's gradients take the f64 forward as y; the kernels' take their own f32 forward, as a caller's do)
    ratios = [cases.assert_under_bar(got, want[name], f"{what} {name}") for got, name in zip(full, ("grad_x", "grad_a1", "grad_a2"))]
    first, second = (np.s_[:, :1], np.s_[:, :2]) if causal else (np.s_[:, -1:], np.s_[:, -2:])
    assert np.all(bits(full[1][first]) == 0) and np.all(bits(full[2][second]) == 0), f"{what}: the masked coefficients' gradients are not +0"
    return forward, max(ratios)


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
    """r inside [0.998, 0.9995]: a group's P is 3e-4 .. 0.13, so the matrix half of var2_carry_1d reaches the result -- four groups,
    66 groups (a second wave), and 1026 (a second sweep; cuts 20,000 .. 40,000 samples apart, none near a sweep boundary).  The seeds
    are the ones under which the numpy replay is at or below half the bar (cases.LONG_MEMORY_SEEDS)"""
    check_all(n, lines, kind, causal)


def test_the_long_memory_cases_are_the_host_tests():
    """the cases above are the ones tests/test_var2_host.py holds the numpy replay to half the bar on and
    tests/test_var2_carry_seen_host.py shows a wrong carry stage on"""
    assert cases.LONG_MEMORY_CASES == [(12292, 1, "long memory"), (266244, 1, "long memory"), (cases.LONG, 1, "long memory, cut")]
    assert exact.LENGTHS == [12292, 266244, cases.LONG] and list(exact.FAMILIES) == ["period 6", "period 3", "running sum"]


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
def check_exact(n, signals, want, causal, what, stride=None):
    """execute and backward on integer signals (lines, n) against the integers of tests/var2_exact.py: no tolerance"""
    x, a1, a2, g = signals
    lines = x.shape[0]
    y = run_forward(n, lines, causal, x, a1, a2, stride)
    exact.assert_equal(y, want["out"], f"{what} out", causal)
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        only_x = run_backward(plan, a1, a2, y, g, False, stride)
        full = run_backward(plan, a1, a2, y, g, True, stride)
    np.testing.assert_array_equal(bits(only_x[0]), bits(full[0]))
    for got, name in zip(full, ("grad_x", "grad_a1", "grad_a2")):
        exact.assert_equal(got, want[name], f"{what} {name}", causal)
    first, second = (np.s_[:, :1], np.s_[:, :2]) if causal else (np.s_[:, -1:], np.s_[:, -2:])
    assert np.all(bits(full[1][first]) == 0) and np.all(bits(full[2][second]) == 0), f"{what}: the masked coefficients' gradients are not +0"


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("family", list(exact.FAMILIES))
@pytest.mark.parametrize("n", exact.LENGTHS)
def test_integer_rotations_are_exact(n, family, causal):
    """constant coefficients whose companion matrix has period 6 or 3, or is the running sum's, on inputs in {-1, 0, 1}: every
    state and every entry of a group's P is a small integer that never decays, so the result is the integer one bit for bit
    whatever the order of operations -- at four groups (the first P_B E_A of either direction), 66 (the fold of the waves'
    totals) and 1026 (the state kept between two sweeps)"""
    check_exact(n, exact.case(n, family, causal), exact.expected(n, family, causal), causal, f"{n} {family} {name_of(causal)}")


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_integer_rotations_on_lines_with_a_stride_above_the_length(causal):
    """one line per family, rows further apart than they are long"""
    n = exact.LENGTHS[0]
    signals = [np.concatenate(s) for s in zip(*(exact.case(n, family, causal) for family in exact.FAMILIES))]
    want = {name: np.concatenate([exact.expected(n, family, causal)[name] for family in exact.FAMILIES]) for name in ("out", "grad_x", "grad_a1", "grad_a2")}
    check_exact(n, signals, want, causal, f"{n} x 3 {name_of(causal)}", stride=n + 12)


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [68, 8196, cases.LONG])
def test_coefficients_of_zero_leave_the_signal(n, causal):
    x = cases.case(n, 1, "sprinkled" if n == cases.LONG else "resonator", causal)[0]
    zero = np.zeros_like(x)
    np.testing.assert_array_equal(bits(run_forward(n, 1, causal, x, zero, zero)), bits(x))


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_constant_coefficients_agree_with_the_order_2_plan(causal):
    """a1 = -2 r cos(theta), a2 = r^2 held constant: rf_plan's order-2 scan (feed-forward 1, feedback -a1, -a2) on the same signal"""
    import torch
    n, r, theta = 8196, 0.95, 0.7
    c1, c2 = np.float32(-2 * r * np.cos(theta)), np.float32(r * r)
    x = cases.case(n, 1, "resonator", causal)[0]
    a1, a2 = np.full((1, n), c1, np.float32), np.full((1, n), c2, np.float32)
    got = run_forward(n, 1, causal, x, a1, a2)
    with rfa.Plan((n,), [(0, causal, [1.0, -float(c1), -float(c2)])]) as plan:
        const = plan.execute([torch.from_numpy(np.array(x[0])).cuda()])[0]
        torch.cuda.synchronize()
        const = const.cpu().numpy()[None, :]
    import var2_loops as loops
    want = loops.forward(x, a1, a2, causal, np.float64)
    serial = loops.forward(x, a1, a2, causal, np.float32)
    peak = float(np.max(np.abs(x)))
    err32 = float(np.max(np.abs(serial - want))) / peak
    cases.assert_under_bar(got, (want, err32, peak), f"constant coefficients {name_of(causal)}, var2")
    # the two against each other, under the same bar
    cases.assert_under_bar(got, (const.astype(np.float64), err32, peak), f"constant coefficients {name_of(causal)}, var2 against rf_plan order 2")


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_a_nan_in_every_masked_slot_changes_nothing(causal):
    n = 4100
    x, a1, a2, g = cases.case(n, 1, "resonator", causal)
    assert np.isnan(a1).sum() == 1 and np.isnan(a2).sum() == 2
    z1, z2 = np.nan_to_num(a1, nan=0.0), np.nan_to_num(a2, nan=0.0)
    y = run_forward(n, 1, causal, x, a1, a2)
    np.testing.assert_array_equal(bits(y), bits(run_forward(n, 1, causal, x, z1, z2)))
    with rfa.Var2Plan(n, causal=causal) as plan:
        for a, b in zip(run_backward(plan, a1, a2, y, g, True), run_backward(plan, z1, z2, y, g, True)):
            assert not np.isnan(a).any()
            np.testing.assert_array_equal(bits(a), bits(b))


# ---- in place, state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
def test_in_place_equals_out_of_place(causal):
    import torch
    lines, n, stride = cases.LINE_CASES[0]
    x, a1, a2, g = cases.case(n, lines, "resonator", causal)
    a = run_forward(n, lines, causal, x, a1, a2, stride)
    b = run_forward(n, lines, causal, x, a1, a2, stride, inplace=True)
    np.testing.assert_array_equal(bits(a), bits(b))
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        d1, d2, dg = (device_lines(v, stride) for v in (a1, a2, g))
        out_of_place = plan.backward(d1, d2, None, dg)[0]
        in_place = plan.backward(d1, d2, None, dg, dg)[0]
        torch.cuda.synchronize()
        assert in_place.data_ptr() == dg.data_ptr()
        np.testing.assert_array_equal(bits(host(out_of_place, lines)), bits(host(in_place, lines)))


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_runs_agree_and_a_plan_keeps_no_state(causal):
    import torch
    n = 8196
    x, a1, a2, g = cases.case(n, 1, "near one", causal)
    fresh = run_forward(n, 1, causal, x, a1, a2)      # another plan
    with rfa.Var2Plan(n, causal=causal) as plan:
        dx, d1, d2 = (device_lines(v) for v in (x, a1, a2))
        results = [plan.execute(dx, d1, d2)]
        plan.execute(torch.full_like(dx, float("nan")), d1, d2)      # a NaN input in between
        results += [plan.execute(dx, d1, d2) for _ in range(2)]
        torch.cuda.synchronize()
        for r in results[1:]:
            guarded.assert_bits_equal([r.cpu()], [results[0].cpu()], "repeated executes of one plan")
        np.testing.assert_array_equal(bits(host(results[0], 1)), bits(fresh))
        first = run_backward(plan, a1, a2, fresh, g, True)
        plan.execute(torch.full_like(dx, float("nan")), d1, d2)
        for a, b in zip(first, run_backward(plan, a1, a2, fresh, g, True)):
            np.testing.assert_array_equal(bits(a), bits(b))


# ---- guarded planes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [4100, 8196])
def test_guarded_signals(n, causal):
    """the input, the coefficients, the output and the four gradient signals between guards: nothing outside them is read (the
    guards of what is read hold NaN) or written"""
    import torch
    x, a1, a2, g = cases.case(n, 1, "resonator", causal)
    want = cases.expected(n, 1, "resonator", causal)
    (d_x, d_1, d_2, d_g), g_read = guarded.guarded_planes((n,), np.float32, 4, fill=guarded.IN_FILL)
    (d_y, d_gx, d_g1, d_g2), g_written = guarded.guarded_planes((n,), np.float32, 4, fill=guarded.OUT_FILL)
    g_read.load([torch.from_numpy(np.array(a[0])) for a in (x, a1, a2, g)])
    g_read.snapshot()
    with rfa.Var2Plan(n, causal=causal) as plan:
        plan.execute(d_x, d_1, d_2, d_y)
        plan.backward(d_1, d_2, d_y, d_g, d_gx, d_g1, d_g2)
        torch.cuda.synchronize()
    g_written.check_guards("output and gradients")
    g_read.check_unchanged("input, coefficients and grad_out")
    what = f"guarded {n} {name_of(causal)}"
    for t, name in zip((d_y, d_gx, d_g1, d_g2), ("out", "grad_x", "grad_a1", "grad_a2")):
        cases.assert_under_bar(host(t, 1), want[name], f"{what} {name}")


# ---- torch.autograd -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("lines,n", [(1, 4098), (2, 4100), (1, 4097)])
def test_allpole_scan_and_its_gradients(lines, n, causal):
    """allpole_scan(...).backward() against the f64 loops on the unpadded signals; 4098 and 4097 are padded to 4100 -- behind the
    end (causal) or before the start (anticausal) -- and sliced back"""
    import torch
    import var2_loops as loops
    rng = np.random.default_rng(100 * n + lines)
    shape = (lines, n)
    x, g = ((rng.random(shape) * 2 - 1).astype(np.float32) for _ in range(2))
    a1, a2 = cases.coefficients("resonator", shape, rng)
    squeeze = (lambda a: a[0]) if lines == 1 else (lambda a: a)
    dx, d1, d2 = (torch.from_numpy(squeeze(a)).cuda().requires_grad_() for a in (x, a1, a2))
    out = rfa.allpole_scan(dx, d1, d2, causal=causal)
    assert tuple(out.shape) == tuple(dx.shape)
    out.backward(torch.from_numpy(squeeze(g)).cuda())
    torch.cuda.synchronize()
    results = {}
    for dtype in (np.float64, np.float32):
        y = loops.forward(x, a1, a2, causal, dtype)
        results[dtype] = [y, *loops.adjoint(a1, a2, y, g, causal, dtype)]
    got = [out.detach(), dx.grad, d1.grad, d2.grad]
    for t, want, serial, name in zip(got, results[np.float64], results[np.float32], ("out", "grad_x", "grad_a1", "grad_a2")):
        peak = float(np.max(np.abs(x))) if name == "out" else float(np.max(np.abs(want)))
        err32 = float(np.max(np.abs(serial - want))) / peak
        cases.assert_under_bar(host(t, lines), (want, err32, peak), f"allpole_scan {lines} x {n} {name_of(causal)} {name}")
    # the input's gradient alone: three launches, the same bits
    dx2 = torch.from_numpy(squeeze(x)).cuda().requires_grad_()
    rfa.allpole_scan(dx2, d1.detach(), d2.detach(), causal=causal).backward(torch.from_numpy(squeeze(g)).cuda())
    np.testing.assert_array_equal(bits(dx2.grad.cpu().numpy()), bits(dx.grad.cpu().numpy()))


# ---- launch names, argument checks that need a device -----------------------------------------------------------------------------
def test_launch_names_and_call_refusals():
    import torch
    n = 4100
    x = torch.zeros(n, device="cuda")
    a1, a2 = torch.full((n,), -0.5, device="cuda"), torch.full((n,), 0.25, device="cuda")
    with rfa.Var2Plan(n) as plan:
        y, times = plan.execute_timed(x, a1, a2)
        assert [name for name, _ in times] == ["var2_tails_1d", "var2_carry_1d", "var2_pass2_1d"]
        assert all(ms >= 0 for _, ms in times)
        *_, times = plan.backward_timed(a1, a2, None, x)
        assert [name for name, _ in times] == ["var2_adj_tails_1d", "var2_carry_1d", "var2_adj_pass2_1d"]
        *_, times = plan.backward_timed(a1, a2, y, x, None, torch.empty_like(x), torch.empty_like(x))
        assert [name for name, _ in times] == ["var2_adj_tails_1d", "var2_carry_1d", "var2_adj_pass2_1d", "var2_grad_1d"]
        off = torch.zeros(n + 4, device="cuda")[1:1 + n]         # 4 bytes off a 16-byte boundary
        half = torch.zeros(2 * n, device="cuda")
        refused = [
            lambda: plan.execute(x, a1, a2, a1),                                       # a coefficient signal that is the output
            lambda: plan.execute(x, a1, a2, a2),
            lambda: plan.execute(off, a1, a2),
            lambda: plan.execute(half[:n], a1, a2, half[4:n + 4]),                     # out overlaps in without being it
            lambda: plan.backward(a1, a2, y, x, None, torch.empty_like(x), None),      # one coefficient gradient without the other
            lambda: plan.backward(a1, a2, y, x, None, None, torch.empty_like(x)),
            lambda: plan.backward(a1, a2, None, x, None, torch.empty_like(x), torch.empty_like(x)),      # coefficient gradients need out
            lambda: plan.backward(a1, a2, y, x, None, y, torch.empty_like(x)),         # a gradient written over what is read
            lambda: plan.backward(a1, a2, y, x, a1),
        ]
        for i, call in enumerate(refused):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG, i
            assert len(str(e.value)) > 30, i
        torch.cuda.synchronize()


# ---- the C++ front-end ----------------------------------------------------------------------------------------------------------
def test_cpp_frontend_varying2(tmp_path):
    """RecFilterVarying2 on a signal of 12356 samples, realize and gradient in both directions against loops in the C++ file;
    compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_varying2.cpp")
    exe = str(tmp_path / "test_frontend_varying2")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "varying2-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
