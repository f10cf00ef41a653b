"""GPU tests of the direct-form-I section on control-rate frames (rf_var2_plan_execute_biquad_frames / _backward_biquad_frames,
rf_var2_expand_frames: var2_frames_kernel, var2_expand_frames_kernel, var2_frames_grad_kernel and var2_frames_fold_kernel of
kernels_var2_signal.hip, plan_var2.cpp, Var2Plan.execute_biquad_frames / biquad_scan_frames of recfilter_amd/var2.py).

The pin is the expansion: expand_frames is exact where every c[n] is representable, and on the expanded signals the frames calls
are rf_var2_plan_execute_biquad / _backward_biquad BIT FOR BIT -- out, grad_in -- which puts them under that section's bar with no
tolerance of their own.  The frame gradients are the per-sample gradients that call stores, contracted: against their f64
contraction the kernels' f64 sums leave one rounding to f32 and 2^-36 of the absolute sum, a bound a tree in f32 does not meet.
End to end, everything is under the family's bar against the f64 loops of tests/frames_loops.py; cases, seeds and bar:
tests/frames_cases.py (tests/test_frames_host.py holds the numpy replay at half the bar on every case here)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import frames_cases as cases
import frames_loops as loops
import guarded
import recfilter_amd as rfa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = cases.DIRECTIONS
FRAME_NAMES = cases.NAMES[2:]
STRIDES = {(lines, n): stride for lines, n, stride, _ in cases.LINE_CASES}
ALL = [(hop, n, lines, kind, causal) for hop, n, lines in cases.SHAPES for kind in cases.KINDS for causal in DIRECTIONS]


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


def device_frames(a):
    """an (L, F) frame array on the device: (F,) for one line, else rows F + FRAME_PAD apart (NaN between them)"""
    return device_lines(a, np.asarray(a).shape[1] + cases.FRAME_PAD)


def host(t, lines):
    return t.cpu().numpy().reshape(lines, -1)


@functools.lru_cache(maxsize=None)
def run(hop, n, lines, kind, causal):
    """every call of one case, once: the results on the host, shared by the tests below and never written"""
    import torch
    x, frames, g = cases.case(hop, n, lines, kind, causal)
    stride = STRIDES.get((lines, n))
    count = loops.frames_count(n, hop)
    nan_frames = lambda: device_frames(np.full((lines, count), np.nan, np.float32))      # noqa: E731
    r = {}
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        dx, dg, df = device_lines(x, stride), device_lines(g, stride), tuple(device_frames(f) for f in frames)
        y = plan.execute_biquad_frames(dx, df, hop)
        signals = [rfa.expand_frames(f, hop, n, out=plan._like(dx)) for f in df]
        y_signals = plan.execute_biquad(dx, *signals)
        unit = tuple(device_frames(np.full((lines, count), v, np.float32)) for v in (1.0, 0.0, 0.0))
        y_unit = plan.execute_biquad_frames(dx, unit + df[3:], hop)
        y_allpole = plan.execute(dx, *signals[3:])
        only_x, none = plan.backward_biquad_frames(dx, df, hop, None, dg)
        assert none is None
        gin, grads = plan.backward_biquad_frames(dx, df, hop, y, dg, None, tuple(nan_frames() for _ in range(5)))
        gin2, grads2 = plan.backward_biquad_frames(dx, df, hop, y, dg, None, tuple(nan_frames() for _ in range(5)))
        gin_signals, per_sample = plan.backward_biquad(dx, *signals, y_signals, dg, None, tuple(plan._like(dx) for _ in range(5)))
        torch.cuda.synchronize()
        for name, t in (("out", y), ("out signals", y_signals), ("out unit", y_unit), ("out allpole", y_allpole), ("only_x", only_x),
                        ("grad_x", gin), ("grad_x again", gin2), ("grad_x signals", gin_signals)):
            r[name] = host(t, lines)
        for name, a, b, p in zip(FRAME_NAMES, grads, grads2, per_sample):
            r[name], r[name + " again"], r[name + " per sample"] = host(a, lines), host(b, lines), host(p, lines)
    return r


# ---- 1: the expansion -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,n,lines,stride", [(64, 4100, 3, 4112), (256, 4100, 3, 4112), (4096, 8196 + 1000, 1, None), (64, 60, 1, None),
                                                (1024, 4096 + 516, 2, 4096 + 520)])
def test_expansion_is_exact_on_representable_frames(hop, n, lines, stride):
    """frames that are multiples of 2^-8 inside [-2, 2], hops up to 4096: every c[n] is a multiple of 2^-20 below 2^2, an f32, and
    expand_frames equals the f64 formula bit for bit; the lengths end inside an interval and the lines are strided"""
    import torch
    assert n % hop != 0
    count = loops.frames_count(n, hop)
    frames = (np.random.default_rng(hop + n).integers(-512, 513, (lines, count)) / 256.0).astype(np.float32)
    want = loops.expand(frames, hop, n, np.float64)
    assert np.all(want.astype(np.float32) == want)
    out = device_lines(np.full((lines, n), np.nan, np.float32), stride)
    got = rfa.expand_frames(device_frames(frames), hop, n, out=out)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(host(got, lines)), bits(want.astype(np.float32)))
    fresh = rfa.expand_frames(device_frames(frames), hop, n)      # allocated by the call
    np.testing.assert_array_equal(bits(host(fresh, lines)), bits(want.astype(np.float32)))
    if lines > 1:
        assert bool(torch.isnan(out._base[:, n:]).all()), "written between the lines"


def test_expansion_of_a_length_that_is_no_multiple_of_4():
    import torch
    frames = (np.random.default_rng(7).integers(-512, 513, (2, 3)) / 256.0).astype(np.float32)
    got = rfa.expand_frames(torch.from_numpy(frames).cuda(), 64, 101)
    assert tuple(got.shape) == (2, 101)
    np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(loops.expand(frames, 64, 101).astype(np.float32)))


# ---- 2, 3: the identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,n,lines,kind,causal", ALL)
def test_forward_is_the_section_on_the_expanded_signals_bit_for_bit(hop, n, lines, kind, causal):
    r = run(hop, n, lines, kind, causal)
    assert not np.isnan(r["out"]).any()
    np.testing.assert_array_equal(bits(r["out"]), bits(r["out signals"]))
    # b = (1, 0, 0) frames: the all-pole scan on the expanded a1, a2
    np.testing.assert_array_equal(bits(r["out unit"]), bits(r["out allpole"]))


@pytest.mark.parametrize("hop,n,lines,kind,causal", ALL)
def test_grad_in_is_the_sections_on_the_expanded_signals_bit_for_bit(hop, n, lines, kind, causal):
    r = run(hop, n, lines, kind, causal)
    assert not np.isnan(r["grad_x"]).any()
    np.testing.assert_array_equal(bits(r["grad_x"]), bits(r["grad_x signals"]))
    np.testing.assert_array_equal(bits(r["only_x"]), bits(r["grad_x"]))      # with or without the frame gradients


# ---- 4: the contraction -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,n,lines,kind,causal", ALL)
def test_frame_gradients_are_the_f64_contraction_rounded_once(hop, n, lines, kind, causal):
    """g32: the per-sample gradients rf_var2_plan_backward_biquad stores on the expanded signals; s = contract(g32) in f64.
    |got - s| <= 2 (2^-24 |s| + 2^-36 sum |w g32|): one rounding to f32, and f64 sums of at most 2^17 exact products"""
    r = run(hop, n, lines, kind, causal)
    count = loops.frames_count(n, hop)
    for name in FRAME_NAMES:
        g32 = r[name + " per sample"]
        s = loops.contract(g32, hop, count, np.float64)
        bound = 2 * (2.0 ** -24 * np.abs(s) + 2.0 ** -36 * loops.contraction_bound(g32, hop, count))
        err = np.abs(r[name].astype(np.float64) - s)
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        print(f"hop {hop} {n} x {lines} {kind} {name_of(causal)} {name}: worst |got - s| / bound {worst:.3f}")
        assert r[name].shape == (lines, count) and not np.isnan(r[name]).any()
        assert np.all(err <= bound), f"{name}: |got - s| up to {worst:.2f} x the bound"


# ---- 5: end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,n,lines,kind,causal", ALL)
def test_against_f64_loops(hop, n, lines, kind, causal):
    r = run(hop, n, lines, kind, causal)
    want = cases.expected(hop, n, lines, kind, causal)
    for name in cases.NAMES:
        cases.assert_under_bar(r[name], want[name], f"hop {hop} {n} x {lines} {kind} {name_of(causal)} {name}")


# ---- 6: reproducibility and footprint -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,n,lines,kind,causal", ALL)
def test_two_backward_calls_give_the_same_bits(hop, n, lines, kind, causal):
    r = run(hop, n, lines, kind, causal)
    for name in cases.NAMES[1:]:
        np.testing.assert_array_equal(bits(r[name]), bits(r[name + " again"]))


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("hop,n", [(64, 4100), (4096, 8196)])
def test_guarded_signals_and_frames(hop, n, causal):
    """x, grad_out and the frame arrays between NaN guards, out, grad_in and the frame gradients between guards: the results are
    the unguarded run's bit for bit, nothing outside is written, and nothing that is read changes"""
    import torch
    x, frames, g = cases.case(hop, n, 1, "resonator", causal)
    count = loops.frames_count(n, hop)
    r = run(hop, n, 1, "resonator", causal)
    read, g_read = guarded.guarded_planes((n,), np.float32, 2, fill=guarded.IN_FILL)
    fread, g_fread = guarded.guarded_planes((count,), np.float32, 5, fill=guarded.IN_FILL)
    written, g_written = guarded.guarded_planes((n,), np.float32, 2, fill=guarded.OUT_FILL)
    fwritten, g_fwritten = guarded.guarded_planes((count,), np.float32, 5, fill=guarded.OUT_FILL)
    g_read.load([torch.from_numpy(np.array(a[0])) for a in (x, g)])
    g_fread.load([torch.from_numpy(np.array(f[0])) for f in frames])
    g_read.snapshot()
    g_fread.snapshot()
    with rfa.Var2Plan(n, causal=causal) as plan:
        plan.execute_biquad_frames(read[0], tuple(fread), hop, written[0])
        plan.backward_biquad_frames(read[0], tuple(fread), hop, written[0], read[1], written[1], tuple(fwritten))
        torch.cuda.synchronize()
    g_written.check_guards("out and grad_in")
    g_fwritten.check_guards("frame gradients")
    g_read.check_unchanged("x and grad_out")
    g_fread.check_unchanged("frames")
    for t, name in zip(list(written) + list(fwritten), cases.NAMES):
        np.testing.assert_array_equal(bits(host(t, 1)), bits(r[name]), err_msg=name)


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_a_nan_in_one_line_reaches_no_other_line(causal):
    import torch
    lines, n, stride, hop = cases.LINE_CASES[0]
    x, frames, g = cases.case(hop, n, lines, "resonator", causal)
    r = run(hop, n, lines, "resonator", causal)
    count = loops.frames_count(n, hop)
    poisoned = np.array(x)
    poisoned[1, n // 2] = np.nan
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        dx, dg, df = device_lines(poisoned, stride), device_lines(g, stride), tuple(device_frames(f) for f in frames)
        y = plan.execute_biquad_frames(dx, df, hop)
        grads = tuple(device_frames(np.full((lines, count), np.nan, np.float32)) for _ in range(5))
        gin, grads = plan.backward_biquad_frames(dx, df, hop, y, dg, None, grads)
        torch.cuda.synchronize()
    got = dict(zip(cases.NAMES, [host(t, lines) for t in (y, gin, *grads)]))
    assert np.isnan(got["out"][1]).any() and np.isnan(got["grad_b0"][1]).any()
    for name in cases.NAMES:
        for line in (0, 2):
            np.testing.assert_array_equal(bits(got[name][line]), bits(r[name][line]), err_msg=f"{name} line {line}")


# ---- 7: the front-ends ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("lines,n,hop", [(1, 5, 64), (2, 4101, 64), (3, 1030, 256)])
def test_biquad_scan_frames_against_biquad_scan_on_lerp_expanded_coefficients(lines, n, hop, causal):
    """biquad_scan_frames(...).backward() under the bar against the f64 loops, beside the route it replaces -- torch.lerp of the
    frames up to audio rate, biquad_scan, autograd back to the frames -- under the same bar; N is no multiple of 4 and the
    gradients reach (L, F) leaves"""
    import torch
    rng = np.random.default_rng(1000 * n + lines)
    count = loops.frames_count(n, hop)
    x, g = ((rng.random((lines, n)) * 2 - 1).astype(np.float32) for _ in range(2))
    frames = cases.frames_of("resonator", lines, count, hop, rng)
    results = {}
    for dtype in (np.float64, np.float32):
        y = loops.forward(x, frames, hop, causal, dtype)
        results[dtype] = [y, *loops.adjoint(x, frames, hop, y, g, causal, dtype)]
    want = cases.biquad_cases.figures(results[np.float64], results[np.float32],
                                      cases.biquad_loops.feed_forward(x, *loops.expand_all(frames, hop, n)[:3], causal, np.float64))
    squeeze = (lambda a: a[0]) if lines == 1 else (lambda a: a)
    dg = torch.from_numpy(squeeze(g)).cuda()

    def leaves():
        return [torch.from_numpy(squeeze(a)).cuda().requires_grad_() for a in (x, *frames)]
    d = leaves()
    out = rfa.biquad_scan_frames(*d, hop, causal=causal)
    assert tuple(out.shape) == tuple(d[0].shape)
    out.backward(dg)
    e = leaves()
    at = torch.arange(n, device="cuda")
    j, w = at // hop, ((at % hop).to(torch.float32) / hop)
    expanded = [torch.lerp(f[..., j], f[..., j + 1], w) for f in e[1:]]
    old = rfa.biquad_scan(e[0], *expanded, causal=causal)
    old.backward(dg)
    torch.cuda.synchronize()
    for a, b, name in zip([out.detach()] + [t.grad for t in d], [old.detach()] + [t.grad for t in e], cases.NAMES):
        assert tuple(a.shape) == ((n,) if name in ("out", "grad_x") else (count,)) if lines == 1 else a.shape[0] == lines
        cases.assert_under_bar(host(a, lines), want[name], f"biquad_scan_frames {lines} x {n} hop {hop} {name_of(causal)} {name}")
        cases.assert_under_bar(host(b, lines), want[name], f"lerp and biquad_scan {lines} x {n} hop {hop} {name_of(causal)} {name}")
    # the input's gradient alone: the same bits
    x2 = torch.from_numpy(squeeze(x)).cuda().requires_grad_()
    rfa.biquad_scan_frames(x2, *(t.detach() for t in d[1:]), hop, causal=causal).backward(dg)
    np.testing.assert_array_equal(bits(x2.grad.cpu().numpy()), bits(d[0].grad.cpu().numpy()))


def test_launch_names_queries_and_call_refusals():
    import torch
    n, hop = 4100, 64
    count = rfa.frames_count(n, hop)
    x = torch.zeros(n, device="cuda")
    frames = tuple(torch.full((count,), v, device="cuda") for v in (1.0, -0.5, 0.25, -0.5, 0.25))
    new = lambda: torch.empty(count, device="cuda")      # noqa: E731
    with rfa.Var2Plan(n) as plan:
        assert plan.backward_biquad_frames_bytes(hop) == 4 * n + 80 * 65
        y, times = plan.execute_biquad_frames_timed(x, frames, hop)
        assert [name for name, _ in times] == ["var2_biquad_frames_tails_1d", "var2_carry_1d", "var2_frames_pass2_1d"]
        assert plan.biquad_frames_num_kernels == 3 and all(ms >= 0 for _, ms in times)
        backward = ["var2_adj_frames_tails_1d", "var2_carry_1d", "var2_adj_frames_pass2_1d", "var2_biquad_frames_grad_1d"]
        *_, times = plan.backward_biquad_frames_timed(x, frames, hop, None, x)
        assert [name for name, _ in times] == backward and plan.backward_biquad_frames_num_kernels(False) == 4
        *_, times = plan.backward_biquad_frames_timed(x, frames, hop, y, x, None, tuple(new() for _ in range(5)))
        assert [name for name, _ in times] == backward + ["var2_frames_fold_1d"] and plan.backward_biquad_frames_num_kernels(True) == 5
        g = torch.ones(n, device="cuda")
        gin, _ = plan.backward_biquad_frames(x, frames, hop, None, g, g)      # grad_in == grad_out is allowed
        assert gin.data_ptr() == g.data_ptr()
        # a smaller hop after a larger one: the slab is regrown
        big = tuple(torch.full((rfa.frames_count(n, 4096),), v, device="cuda") for v in (1.0, -0.5, 0.25, -0.5, 0.25))
        plan.backward_biquad_frames(x, big, 4096, y, g, None, tuple(torch.empty_like(t) for t in big))
        plan.backward_biquad_frames(x, frames, hop, y, g, None, tuple(new() for _ in range(5)))
        refused = [
            lambda: plan.execute_biquad_frames(x, frames, hop, x),                                            # in == out
            lambda: plan.backward_biquad_frames(x, frames, hop, None, g, None, tuple(new() for _ in range(5))),      # frame gradients need out
            lambda: plan.backward_biquad_frames(x, frames, hop, y, g, x),                                     # a gradient written over what is read
            lambda: plan.backward_biquad_frames(x, frames, hop, y, g, None, frames),                          # frame gradients over the frames
        ]
        for i, call in enumerate(refused):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG, i
            assert len(str(e.value)) > 30, i
        for call in (lambda: plan.execute_biquad_frames(x, frames, 480), lambda: plan.execute_biquad_frames(x, frames[:4], hop),
                     lambda: plan.execute_biquad_frames(x, tuple(f[:-1] for f in frames), hop)):
            with pytest.raises(ValueError):
                call()
        torch.cuda.synchronize()


# ---- 8: the C++ front-end -------------------------------------------------------------------------------------------------------------
def test_cpp_frontend_biquad_frames(tmp_path):
    """RecFilterVarying2::realize_biquad_frames / gradient_biquad_frames on a signal of 12356 samples at hops 64 and 8192, both
    directions, against loops in the C++ file; compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_biquad_frames.cpp")
    exe = str(tmp_path / "test_frontend_biquad_frames")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "biquad-frames-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
