"""GPU tests of cascades of time-varying direct-form-I sections (rf_var2_plan_execute_cascade / _backward_cascade: var2_link_1d
and var2_link_keep_1d of kernels_var2_signal.hip, plan_var2.cpp, Var2Plan.execute_cascade / biquad_cascade of
recfilter_amd/var2.py).

Reference: the f64 loops of tests/cascade_loops.py (pinned against central differences in tests/test_cascade_host.py); cases and
bar: tests/cascade_cases.py -- max abs error over the peak <= max(4 x the same figure of the numpy f32 serial cascade, 1e-6), the
forward and all 1 + 5 K gradients.  tests/test_cascade_host.py holds the numpy replay of the kernels to half that bar on every
case here.  Every coefficient a section masks holds NaN; inputs are seeded, signed, in [-1, 1].

The exact identities pin the link: with all feedback coefficients 0 the stored maps reproduce the samples exactly, the state
that enters a tile IS the neighbouring tile's two samples, and the cascade is K successive execute_biquad calls bit for bit."""
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


def same_bits(a, b, what=""):
    """np.array_equal on the values: +0 and -0 are not told apart"""
    assert np.array_equal(np.asarray(a), np.asarray(b)), what


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


def run_forward(plan, x, sections, stride=None):
    import torch
    out = plan.execute_cascade(device_lines(x, stride), device_sections(sections, stride))
    torch.cuda.synchronize()
    return host(out, np.asarray(x).shape[0])


def run_backward(plan, x, sections, y, g, with_coefficients, stride=None):
    """[grad_x, then the 5 K coefficient gradients] on the host (grad_x alone without them); what the call writes is NaN before"""
    import torch
    shape = np.asarray(g).shape
    grads = None
    if with_coefficients:
        grads = [tuple(device_lines(np.full(shape, np.nan, np.float32), stride) for _ in range(5)) for _ in sections]
    gin, grads = plan.backward_cascade(device_lines(x, stride), device_sections(sections, stride),
                                       device_lines(y, stride) if with_coefficients else None, device_lines(g, stride), None, grads)
    torch.cuda.synchronize()
    return [host(t, shape[0]) for t in [gin] + [t for s in (grads or ()) for t in s]]


def assert_masked_gradients_are_zero(full, causal, K, what):
    one, two = (np.s_[:, :1], np.s_[:, :2]) if causal else (np.s_[:, -1:], np.s_[:, -2:])
    for k in range(K):
        gb1, gb2, ga1, ga2 = full[1 + 5 * k + 1], full[1 + 5 * k + 2], full[1 + 5 * k + 3], full[1 + 5 * k + 4]
        for grad, where in ((gb1, one), (gb2, two), (ga1, one), (ga2, two)):
            assert np.all(bits(grad[where]) == 0), f"{what}: the masked coefficients' gradients of section {k} are not +0"


def check_all(n, lines, kind, causal, K, stride=None):
    """the forward and the backward without and with coefficient gradients of one case under the bar"""
    x, sections, g = cases.case(n, lines, kind, causal, K)
    want = cases.expected(n, lines, kind, causal, K)
    what = f"{n} x {lines} {kind} K={K} {name_of(causal)}"
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        y = run_forward(plan, x, sections, stride)
        cases.assert_under_bar(y, want["out"], f"{what} out")
        only_x = run_backward(plan, x, sections, y, g, False, stride)
        full = run_backward(plan, x, sections, y, g, True, stride)
    assert len(only_x) == 1 and len(full) == 1 + 5 * K
    np.testing.assert_array_equal(bits(only_x[0]), bits(full[0]))      # with or without the coefficient gradients
    for got, name in zip(full, cases.names(K)[1:]):
        cases.assert_under_bar(got, want[name], f"{what} {name}")
    assert_masked_gradients_are_zero(full, causal, K, what)


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
def test_long_signal_against_segmented_loops(causal):
    """4,198,404 samples, 1026 groups: var2_carry_1d takes two sweeps between the links"""
    check_all(cases.LONG, 1, "sprinkled", causal, 2)


def test_the_accuracy_cases_are_the_host_tests():
    """the cases above are cases.GPU_CASES, the ones tests/test_cascade_host.py holds the numpy replay to half the bar on"""
    here = ([(n, 1, kind, K) for K in (1, 2, 4) for n in cases.LENGTHS for kind in cases.KINDS]
            + [(n, 1, kind, 8) for n in (4100, 8196) for kind in ("resonator", "sprinkled")]
            + [(n, lines, "resonator", 2) for lines, n, _ in cases.LINE_CASES] + [(cases.LONG, 1, "sprinkled", 2)])
    assert here == cases.GPU_CASES


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n,lines,kind,K", cases.LONG_MEMORY_CASES)
def test_long_memory_against_f64_loops(n, lines, kind, K, causal):
    """r inside [0.998, 0.9995] at four groups, K = 2: a group's P reaches the result through var2_link_1d and var2_link_keep_1d
    (tests/var2_cases.py); the seeds are the ones under which the numpy replay meets the host test's condition"""
    assert cases.LONG_MEMORY_CASES == [(12292, 1, "long memory", 2)]      # the ones tests/test_cascade_host.py holds the replay on
    check_all(n, lines, kind, causal, K)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", exact.LENGTHS[:2])
def test_integer_rotations_of_two_periods_are_exact(n, causal):
    """tests/var2_exact.py: a section of period 6 into one of period 3 (two of one period would resonate and grow), integer taps,
    inputs in {-1, 0, 1}: the state that enters every tile of the link is an integer that never decayed, and the output and the
    gradients are the integers bit for bit, at four groups and at 66.  Every one of the 11 gradients is checked: all stay below
    2^24 at these lengths (the reference says which do not, and none may be left out silently)"""
    x, sections, g = exact.cascade_case(n, causal)
    want, left_out = exact.cascade_expected(n, causal)
    assert not left_out, f"gradients that reach 2^24 and could not be compared: {left_out}"
    what = f"{n} period 6 into period 3 {name_of(causal)}"
    with rfa.Var2Plan(n, causal=causal) as plan:
        y = run_forward(plan, x, sections)
        exact.assert_equal(y, want["out"], f"{what} out", causal)
        only_x = run_backward(plan, x, sections, y, g, False)
        full = run_backward(plan, x, sections, y, g, True)
    np.testing.assert_array_equal(bits(only_x[0]), bits(full[0]))
    for got, name in zip(full, cases.names(2)[1:]):
        exact.assert_equal(got, want[name], f"{what} {name}", causal)
    assert_masked_gradients_are_zero(full, causal, 2, what)


# ---- exact identities -------------------------------------------------------------------------------------------------------------
def unit_section(shape):
    one, zero = np.ones(shape, np.float32), np.zeros(shape, np.float32)
    return (one, zero, zero, zero, zero)


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [68, 8196])
def test_one_section_is_execute_biquad(n, causal):
    import torch
    x, sections, _ = cases.case(n, 1, "resonator", causal, 1)
    with rfa.Var2Plan(n, causal=causal) as plan:
        got = run_forward(plan, x, sections)
        want = plan.execute_biquad(device_lines(x), *device_sections(sections)[0])
        torch.cuda.synchronize()
    same_bits(got, host(want, 1))


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [68, 4100, 8196])
def test_identity_sections_change_no_bit(n, causal):
    """trailing sections with b = (1, 0, 0), a = (0, 0) give the shorter cascade's bits, and so does a leading one: with zero
    feedback the stored maps reproduce the samples exactly"""
    x, sections, _ = cases.case(n, 1, "resonator", causal, 2)
    unit = unit_section(x.shape)
    with rfa.Var2Plan(n, causal=causal) as plan:
        want = run_forward(plan, x, sections)
        same_bits(run_forward(plan, x, sections + (unit,)), want, "one trailing identity section")
        same_bits(run_forward(plan, x, sections + (unit, unit, unit)), want, "three trailing identity sections")
        same_bits(run_forward(plan, x, (unit,) + sections), want, "a leading identity section")


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [64, 68, 4096, 4100, 8196])
def test_zero_feedback_is_successive_execute_biquad_calls(n, causal):
    """all a = 0: the cascade equals K successive execute_biquad calls bit for bit -- the link's neighbour indexing at tile and
    group edges"""
    import torch
    K = 4
    x, sections, _ = cases.case(n, 1, "resonator", causal, K)
    zero = np.zeros_like(x)
    sections = tuple((b0, b1, b2, zero, zero) for b0, b1, b2, _, _ in sections)
    with rfa.Var2Plan(n, causal=causal) as plan:
        got = run_forward(plan, x, sections)
        t = device_lines(x)
        for s in device_sections(sections):
            t = plan.execute_biquad(t, *s)
        torch.cuda.synchronize()
    same_bits(got, host(t, 1))


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_a_nan_in_every_masked_slot_changes_nothing(causal):
    n, K = 4100, 4
    x, sections, g = cases.case(n, 1, "resonator", causal, K)
    assert all([int(np.isnan(c).sum()) for c in s] == [0, 1, 2, 1, 2] for s in sections)
    cleared = tuple(tuple(np.nan_to_num(c, nan=0.0) for c in s) for s in sections)
    with rfa.Var2Plan(n, causal=causal) as plan:
        y = run_forward(plan, x, sections)
        np.testing.assert_array_equal(bits(y), bits(run_forward(plan, x, cleared)))
        full = run_backward(plan, x, sections, y, g, True)
        for a, b in zip(full, run_backward(plan, x, cleared, y, g, True)):
            assert not np.isnan(a).any()
            np.testing.assert_array_equal(bits(a), bits(b))
    assert_masked_gradients_are_zero(full, causal, K, f"NaN in the masked slots, {name_of(causal)}")


# ---- state, guards ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
def test_runs_agree_and_a_plan_keeps_no_state(causal):
    import torch
    n, K = 8196, 4
    x, sections, g = cases.case(n, 1, "near one", causal, K)
    with rfa.Var2Plan(n, causal=causal) as other:
        fresh = run_forward(other, x, sections)
    with rfa.Var2Plan(n, causal=causal) as plan:
        dx, ds = device_lines(x), device_sections(sections)
        poison = torch.full_like(dx, float("nan"))
        results = [plan.execute_cascade(dx, ds)]
        plan.execute_cascade(poison, ds)      # a NaN input in between
        results += [plan.execute_cascade(dx, ds) for _ in range(2)]
        torch.cuda.synchronize()
        for r in results[1:]:
            guarded.assert_bits_equal([r.cpu()], [results[0].cpu()], "repeated executes of one plan")
        np.testing.assert_array_equal(bits(host(results[0], 1)), bits(fresh))
        # a backward at K = 4, then K = 2, then K = 4 again (the plan's signals are allocated, kept, and used again), a NaN
        # gradient through them in between
        first = run_backward(plan, x, sections, fresh, g, True)
        assert plan.backward_cascade_bytes(4) == 5 * 4 * n and plan.backward_cascade_bytes(2) == 3 * 4 * n
        two = run_forward(plan, x, sections[:2])
        short = run_backward(plan, x, sections[:2], two, g, True)
        plan.backward_cascade(dx, ds, None, poison)
        for a, b in zip(first, run_backward(plan, x, sections, fresh, g, True)):
            np.testing.assert_array_equal(bits(a), bits(b))
    # the regrowth: K = 2 first on a new plan, then K = 4
    with rfa.Var2Plan(n, causal=causal) as plan:
        for a, b in zip(short, run_backward(plan, x, sections[:2], two, g, True)):
            np.testing.assert_array_equal(bits(a), bits(b))
        for a, b in zip(first, run_backward(plan, x, sections, fresh, g, True)):
            np.testing.assert_array_equal(bits(a), bits(b))


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [68, 4100])
def test_guarded_signals(n, causal):
    """the input, the ten coefficients and grad_out, the output and the eleven gradients between guards: nothing outside them is
    read (the guards of what is read hold NaN) or written"""
    import torch
    K = 2
    x, sections, g = cases.case(n, 1, "resonator", causal, K)
    want = cases.expected(n, 1, "resonator", causal, K)
    read, g_read = guarded.guarded_planes((n,), np.float32, 2 + 5 * K, fill=guarded.IN_FILL)
    written, g_written = guarded.guarded_planes((n,), np.float32, 2 + 5 * K, fill=guarded.OUT_FILL)
    g_read.load([torch.from_numpy(np.array(a[0])) for a in (x, g, *(c for s in sections for c in s))])
    g_read.snapshot()
    ds = [tuple(read[2 + 5 * k:7 + 5 * k]) for k in range(K)]
    grads = [tuple(written[2 + 5 * k:7 + 5 * k]) for k in range(K)]
    with rfa.Var2Plan(n, causal=causal) as plan:
        plan.execute_cascade(read[0], ds, written[0])
        plan.backward_cascade(read[0], ds, written[0], read[1], written[1], grads)
        torch.cuda.synchronize()
    g_written.check_guards("output and gradients")
    g_read.check_unchanged("input, coefficients and grad_out")
    for t, name in zip(written, cases.names(K)):
        cases.assert_under_bar(host(t, 1), want[name], f"guarded {n} {name_of(causal)} {name}")


# ---- front-ends -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("lines,n", [(1, 5), (2, 4101)])
def test_biquad_cascade_and_its_gradients(lines, n, causal):
    """biquad_cascade(...).backward() against the f64 loops on the unpadded signals -- 5 is padded to 8 and 4101 to 4104, behind
    the end (causal) or before the start (anticausal), and sliced back -- and K chained biquad_scan calls under the same bar"""
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
    out = rfa.biquad_cascade(dx, ds, causal=causal)
    assert tuple(out.shape) == tuple(dx.shape)
    out.backward(dg)
    cx, cs = leaves()
    chained = cx
    for s in cs:
        chained = rfa.biquad_scan(chained, *s, causal=causal)
    chained.backward(dg)
    torch.cuda.synchronize()
    fused = [out.detach(), dx.grad] + [c.grad for s in ds for c in s]
    separate = [chained.detach(), cx.grad] + [c.grad for s in cs for c in s]
    for a, b, name in zip(fused, separate, cases.names(K)):
        cases.assert_under_bar(host(a, lines), want[name], f"biquad_cascade {lines} x {n} {name_of(causal)} {name}")
        cases.assert_under_bar(host(b, lines), want[name], f"chained biquad_scan {lines} x {n} {name_of(causal)} {name}")
    # the input's gradient alone: the same bits
    x2 = torch.from_numpy(squeeze(x)).cuda().requires_grad_()
    rfa.biquad_cascade(x2, [tuple(c.detach() for c in s) for s in ds], causal=causal).backward(dg)
    np.testing.assert_array_equal(bits(x2.grad.cpu().numpy()), bits(dx.grad.cpu().numpy()))


def test_launch_names_counts_and_call_refusals():
    import torch
    n = 4100
    x = torch.zeros(n, device="cuda")
    new = lambda: torch.empty_like(x)      # noqa: E731
    section = tuple(torch.full((n,), v, device="cuda") for v in (1.0, -0.5, 0.25, -0.5, 0.25))
    adjoint = ["var2_adj_tails_1d", "var2_carry_1d", "var2_adj_pass2_1d", "var2_biquad_grad_1d"]
    with rfa.Var2Plan(n) as plan:
        for K in (1, 2, 3, 16):
            sections = [section] * K
            y, times = plan.execute_cascade_timed(x, sections)
            want = ["var2_biquad_tails_1d"] + ["var2_carry_1d", "var2_link_1d"] * (K - 1) + ["var2_carry_1d", "var2_pass2_1d"]
            assert [name for name, _ in times] == want and len(want) == 2 * K + 1 == plan.cascade_num_kernels(K)
            assert all(ms >= 0 for _, ms in times)
            rerun = [] if K == 1 else (["var2_biquad_tails_1d"] + ["var2_carry_1d", "var2_link_keep_1d"] * (K - 2) + ["var2_carry_1d", "var2_pass2_1d"])
            want = rerun + adjoint * K
            assert len(want) == (4 if K == 1 else 6 * K - 1) == plan.backward_cascade_num_kernels(K)
            *_, times = plan.backward_cascade_timed(x, sections, None, x)
            assert [name for name, _ in times] == want
            *_, times = plan.backward_cascade_timed(x, sections, y, x, None, [tuple(new() for _ in range(5)) for _ in range(K)])
            assert [name for name, _ in times] == want
        g = torch.ones(n, device="cuda")
        gin, _ = plan.backward_cascade(x, [section] * 2, None, g, g)      # grad_in == grad_out is allowed
        assert gin.data_ptr() == g.data_ptr()
        two = [section, section]
        refused = [
            lambda: plan.execute_cascade(x, two, x),                                             # in == out
            lambda: plan.execute_cascade(x, two, section[1]),                                    # a coefficient signal that is the output
            lambda: plan.execute_cascade(x, []),                                                 # no section
            lambda: plan.execute_cascade(x, [section] * 17),                                     # too many
            lambda: plan.execute_cascade(torch.zeros(n + 4, device="cuda")[1:1 + n], two),       # 4 bytes off a 16-byte boundary
            lambda: plan.backward_cascade(x, two, y, g, None, [tuple(new() for _ in range(5)), (new(), new(), None, new(), new())]),
            lambda: plan.backward_cascade(x, two, None, g, None, [tuple(new() for _ in range(5)) for _ in range(2)]),      # gradients need out
            lambda: plan.backward_cascade(x, two, y, g, x),                                      # a gradient written over what is read
        ]
        for i, call in enumerate(refused):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG, i
            assert len(str(e.value)) > 15, i
        torch.cuda.synchronize()


def test_cpp_frontend_cascade(tmp_path):
    """RecFilterVarying2::realize_cascade / gradient_cascade on a signal of 12356 samples, both directions, against loops in the
    C++ file; compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_cascade.cpp")
    exe = str(tmp_path / "test_frontend_cascade")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "cascade-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
