"""GPU tests of the varying scans on long 1-D signals (rf_var_plan_create_signal: kernels_var_signal.hip, plan_var.cpp,
VarPlan.signal / var_scan_signal / smooth_samples of recfilter_amd/varscan.py).

Reference: the f64 serial loops of tests/test_gpu_var_scans.py on (1, N) arrays; bar and printout are that file's: max abs error
over the input peak <= max(4 x the same figure of the numpy f32 serial loop, 1e-6).  Gradients: the f64 loops of
tests/var_grad_loops.py and tests/smooth_grad_loops.py (pinned by central differences in tests/test_var_grad_host.py,
tests/test_smooth_grad_host.py and, on a signal, tests/test_var_signal_host.py) under the bar of tests/test_gpu_var_grad.py.
Weight signals hold NaN at element 0; inputs are seeded, signed, in [-1, 1].

The long case, 8,388,936 = 2 * 1024 * 4096 + 5 * 64 + 8 samples, is 2049 groups: var_carry_1d takes three sweeps of sixteen waves.
Its weights hold exact zeros at irregular gaps of 3000..8191 samples; a weight of 0 decouples exactly in both directions, so the
signal splits into independent segments and the serial loops run vectorised over them, the segments taken in buckets of similar
length (the 1 % sprinkling of exact zeros and ones at the long length: 84,000 segments, most of them shorter than 128 samples)."""
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import guarded
import smooth_grad_loops as power_loops
import var_grad_cases as grad_cases
import var_grad_loops as loops
import recfilter_amd as rfa
from test_gpu_var_scans import assert_under_bar, reference, to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P0, M0, P1, M1 = (0, True, 0), (0, False, 0), (0, True, 1), (0, False, 1)
SCAN_LISTS = {"+x": [P0], "-x": [M0], "+x-x": [P0, M0], "-x+x": [M0, P0], "+x-x+x": [P0, M0, P0], "+x-x two weights": [P0, M1]}
LENGTHS = [4, 64, 68, 4096, 4100, 12616]
LONG = 2 * 1024 * 4096 + 5 * 64 + 8
BASES = [0.8, 0.97]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def rows(arrays):
    """1-D arrays as the (1, N) planes the reference loops take"""
    return [np.asarray(a)[None, :] for a in arrays]


@functools.lru_cache(maxsize=None)
def case(n, planes, kind="quarter"):
    """(inputs, two weight signals) of a length, seeded; shared and never written.  kind "power": the weights are exponents"""
    rng = np.random.default_rng(zlib.crc32(repr((n, planes, kind)).encode()))
    ins = [(rng.random(n) * 2 - 1).astype(np.float32) for _ in range(planes)]
    if kind == "near one":
        ws = [np.minimum((0.99 + 0.01 * rng.random(n)).astype(np.float32), np.float32(1 - 2.0 ** -24)) for _ in range(2)]
    elif kind == "power":
        ws = [(1.0 + 30.0 * rng.random(n) ** 4).astype(np.float32) for _ in range(2)]
    else:
        ws = [(rng.random(n) ** 0.25).astype(np.float32) for _ in range(2)]
    if kind == "sprinkled":
        for w in ws:
            u = rng.random(n)
            w[u < 0.01] = 0.0
            w[u > 0.99] = 1.0
    for w in ws:
        w[0] = np.nan
    for a in ins + ws:
        a.setflags(write=False)
    return ins, ws


def as_weights(ws, kind, dtype):
    return [power_loops.power_weights(w, b, dtype) for w, b in zip(ws, BASES)] if kind == "power" else ws


@functools.lru_cache(maxsize=None)
def expected(n, planes, name, kind="quarter"):
    """(f64 reference as 1-D arrays, err / peak of the f32 serial loop, input peak)"""
    ins, ws = case(n, planes, kind)
    want = reference(rows(ins), rows(as_weights(ws, kind, np.float64)), SCAN_LISTS[name], np.float64)
    serial = reference(rows(ins), rows(as_weights(ws, kind, np.float32)), SCAN_LISTS[name], np.float32)
    peak = max(float(np.max(np.abs(p))) for p in ins)
    err32 = max(float(np.max(np.abs(s.astype(np.float64) - w))) for s, w in zip(serial, want)) / peak
    return [w[0] for w in want], err32, peak


def run(n, planes, scans, ins, ws, kind="quarter", inplace=False):
    import torch
    with rfa.VarPlan.signal(n, scans, planes=planes, n_weights=2) as plan:
        src = to_device(ins)
        outs = src if inplace else None
        outs = plan.execute_power(src, to_device(ws), BASES, outs) if kind == "power" else plan.execute(src, to_device(ws), outs)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["quarter", "power"])
@pytest.mark.parametrize("name", list(SCAN_LISTS))
@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("n", LENGTHS)
def test_against_f64_loops(n, planes, name, kind):
    ins, ws = case(n, planes, kind)
    want, err32, peak = expected(n, planes, name, kind)
    got = run(n, planes, SCAN_LISTS[name], ins, ws, kind)
    assert_under_bar(got, want, err32, peak, f"{n} x {planes} {name} {kind}")


@pytest.mark.parametrize("name", ["+x-x", "-x+x"])
def test_weights_near_one(name):
    n = 12616
    ins, ws = case(n, 1, "near one")
    want, err32, peak = expected(n, 1, name, "near one")
    assert_under_bar(run(n, 1, SCAN_LISTS[name], ins, ws), want, err32, peak, f"{n} near one {name}")


@pytest.mark.parametrize("name", ["+x", "-x", "+x-x"])
def test_weights_with_exact_zeros_and_ones(name):
    n = 12616
    ins, ws = case(n, 1, "sprinkled")
    assert (ws[0] == 0).any() and (ws[0] == 1).any()
    want, err32, peak = expected(n, 1, name, "sprinkled")
    assert_under_bar(run(n, 1, SCAN_LISTS[name], ins, ws, "sprinkled"), want, err32, peak, f"sprinkled {name}")


# ---- the long case ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_case(kind):
    """(input, weight signal or exponent signal, segment starts) of LONG samples: exact decoupling at gaps of 3000..8191"""
    rng = np.random.default_rng(zlib.crc32(repr(("long", kind)).encode()))
    x = (rng.random(LONG) * 2 - 1).astype(np.float32)
    if kind == "near one":
        w = np.minimum((0.99 + 0.01 * rng.random(LONG)).astype(np.float32), np.float32(1 - 2.0 ** -24))
    elif kind == "power":
        w = (1.0 + 30.0 * rng.random(LONG) ** 4).astype(np.float32)
    else:
        w = (rng.random(LONG) ** 0.25).astype(np.float32)
    if kind == "sprinkled":                                   # exact 0 and exact 1, 1 % each: the zeros are the segment starts
        u = rng.random(LONG)
        w[u < 0.01] = 0.0
        w[u > 0.99] = 1.0
        starts = np.flatnonzero(w == 0)
        starts = starts if starts[0] == 0 else np.concatenate([[0], starts])
    else:
        starts = np.concatenate([[0], np.cumsum(rng.integers(3000, 8192, LONG // 3000 + 1))])
        starts = starts[starts < LONG]
        w[starts] = np.inf if kind == "power" else 0.0
    w[0] = np.nan
    x.setflags(write=False)
    w.setflags(write=False)
    return x, w, starts


@functools.lru_cache(maxsize=None)
def long_expected(name, kind):
    x, w, starts = long_case(kind)
    ends = np.append(starts[1:], LONG)
    lengths = ends - starts
    longest = int(lengths.max())

    def segments(dtype):
        ww = as_weights([w], kind, dtype)[0]
        out = np.empty(LONG, np.float64)
        low = 0
        for width in sorted({min(128, longest), min(512, longest), longest}):      # buckets of similar length, padded to the widest
            pick = (lengths > low) & (lengths <= width)
            low = width
            if not pick.any():
                continue
            at = starts[pick, None] + np.arange(width)[None, :]
            inside = at < ends[pick, None]
            at = np.minimum(at, LONG - 1)
            xs = np.where(inside, x[at], 0).astype(dtype)
            wseg = np.where(inside, ww[at], 0).astype(dtype)      # (a segment's element 0 is never read)
            out[at[inside]] = reference([xs], [wseg], SCAN_LISTS[name], dtype)[0][inside]
        return out
    want = segments(np.float64)
    serial = segments(np.float32)
    peak = float(np.max(np.abs(x)))
    return want, float(np.max(np.abs(serial - want))) / peak, peak


@pytest.mark.parametrize("name,kind", [("+x-x", "quarter"), ("+x-x", "near one"), ("-x+x", "power"), ("+x-x", "sprinkled")])
def test_long_signal_against_segmented_loops(name, kind):
    x, w, _ = long_case(kind)
    want, err32, peak = long_expected(name, kind)
    got = run(LONG, 1, SCAN_LISTS[name], [x], [w, w], kind)
    assert_under_bar(got, [want], err32, peak, f"{LONG} {name} {kind}")


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
def constant_weights(n, value):
    w = np.full(n, value, dtype=np.float32)
    w[0] = np.nan
    return [w, w]


@pytest.mark.parametrize("n", [12616, LONG])
def test_weights_of_zero_leave_the_signal(n):
    x = long_case("quarter")[0][:n]
    for name in ("+x", "-x", "+x-x"):
        got = run(n, 1, SCAN_LISTS[name], [x], constant_weights(n, 0.0))
        assert np.array_equal(bits(got[0]), bits(x)), name


@pytest.mark.parametrize("n", [12616, LONG])
@pytest.mark.parametrize("name,sample", [("+x", 0), ("-x", -1), ("+x-x", 0)])
def test_weights_of_one_spread_one_sample(n, name, sample):
    x = long_case("quarter")[0][:n]
    got = run(n, 1, SCAN_LISTS[name], [x], constant_weights(n, 1.0))[0]
    assert np.array_equal(got, np.full(n, x[sample], dtype=np.float32))


# ---- in place, state ------------------------------------------------------------------------------------------------------------
def test_in_place_equals_out_of_place():
    n, planes = 12616, 3
    ins, ws = case(n, planes)
    a = run(n, planes, SCAN_LISTS["+x-x+x"], ins, ws)
    b = run(n, planes, SCAN_LISTS["+x-x+x"], ins, ws, inplace=True)
    for p, q in zip(a, b):
        np.testing.assert_array_equal(bits(p), bits(q))


def test_a_plan_keeps_no_state():
    import torch
    n, planes = 12616, 1
    ins, ws = case(n, planes)
    scans = SCAN_LISTS["+x-x+x"]
    fresh = run(n, planes, scans, ins, ws)      # another plan
    with rfa.VarPlan.signal(n, scans, planes=planes, n_weights=2) as plan:
        dws = to_device(ws)
        results = [plan.execute(to_device(ins), dws)]
        plan.execute(to_device([np.full(n, np.nan, dtype=np.float32)]), dws)      # a NaN input in between
        results += [plan.execute(to_device(ins), dws) for _ in range(2)]
        torch.cuda.synchronize()
        for r in results[1:]:
            guarded.assert_bits_equal([t.cpu() for t in r], [t.cpu() for t in results[0]], "repeated executes of one plan")
        np.testing.assert_array_equal(bits(results[0][0].cpu().numpy()), bits(fresh[0]))


# ---- guarded planes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,planes", [(4100, 1), (12616, 3)])
def test_guarded_planes(n, planes):
    import torch
    ins, ws = case(n, planes)
    want, err32, peak = expected(n, planes, "+x-x+x")
    d_in, g_in = guarded.guarded_planes((n,), np.float32, planes, fill=guarded.IN_FILL)
    d_w, g_w = guarded.guarded_planes((n,), np.float32, 2, fill=guarded.IN_FILL)
    d_out, g_out = guarded.guarded_planes((n,), np.float32, planes, fill=guarded.OUT_FILL)
    g_in.load([torch.from_numpy(np.array(a)) for a in ins])
    g_w.load([torch.from_numpy(np.array(a)) for a in ws])
    g_in.snapshot()
    g_w.snapshot()
    with rfa.VarPlan.signal(n, SCAN_LISTS["+x-x+x"], planes=planes, n_weights=2) as plan:
        plan.execute(d_in, d_w, d_out)
        torch.cuda.synchronize()
    g_out.check_guards("output")
    g_in.check_unchanged("input")
    g_w.check_unchanged("weights")
    assert_under_bar([o.cpu().numpy() for o in d_out], want, err32, peak, f"guarded {n} x {planes}")


# ---- gradients ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grad_out(n, planes):
    rng = np.random.default_rng(zlib.crc32(repr(("grad_out", n, planes)).encode()))
    return [(rng.random(n) * 2 - 1).astype(np.float32) for _ in range(planes)]


@functools.lru_cache(maxsize=None)
def expected_gradients(n, planes, name, kind):
    """(grad_ins, grad_weights, err32 of grad_ins, [err32 per weight signal]) from the f64 and f32 loops, as (1, N) arrays"""
    ins, ws = case(n, planes, kind)
    g = rows(grad_out(n, planes))

    def both(dtype):
        if kind == "power":
            return power_loops.power_backward(rows(ins), rows(ws), BASES, SCAN_LISTS[name], g, dtype)
        return loops.backward(rows(ins), rows(ws), SCAN_LISTS[name], g, dtype)
    want_in, want_w = both(np.float64)
    ser_in, ser_w = both(np.float32)
    err_w = [None if w is None else grad_cases.figures([s], [w])[0] for s, w in zip(ser_w, want_w)]
    return want_in, want_w, grad_cases.figures(ser_in, want_in)[0], err_w


def run_backward(plan, ins, ws, g, kind, with_weights):
    import torch
    read = {k for _, _, k in plan.scans}
    d_gw = [torch.full((plan.shape[0],), np.nan, device="cuda") if k in read else None for k in range(2)] if with_weights else None
    d_in = to_device(ins) if with_weights else None
    if kind == "power":
        gin, gw = plan.backward_power(d_in, to_device(ws), BASES, to_device(g), None, d_gw)
    else:
        gin, gw = plan.backward(d_in, to_device(ws), to_device(g), None, d_gw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in gin], None if gw is None else [None if t is None else t.cpu().numpy() for t in gw]


@pytest.mark.parametrize("kind", ["quarter", "power"])
@pytest.mark.parametrize("name", list(SCAN_LISTS))
@pytest.mark.parametrize("n,planes", [(68, 1), (4100, 3), (12616, 1)])
def test_gradients_against_f64_loops(n, planes, name, kind):
    ins, ws = case(n, planes, kind)
    g = grad_out(n, planes)
    want_in, want_w, err_in, err_w = expected_gradients(n, planes, name, kind)
    what = f"{n} x {planes} {name} {kind}"
    with rfa.VarPlan.signal(n, SCAN_LISTS[name], planes=planes, n_weights=2) as plan:
        image_only, none = run_backward(plan, ins, ws, g, kind, False)
        gin, gw = run_backward(plan, ins, ws, g, kind, True)
        again_in, again_w = run_backward(plan, ins, ws, g, kind, True)
    assert none is None
    grad_cases.assert_under_bar(rows(gin), want_in, err_in, f"{what} grad_in")
    for k, (got, want, e) in enumerate(zip(gw, want_w, err_w)):
        if want is None:
            assert got is None
            continue
        grad_cases.assert_under_bar(rows([got]), [want], e, f"{what} grad_w[{k}]")
        assert got[0] == 0.0 and not np.signbit(got[0]), f"{what} grad_w[{k}]: element 0 is not exactly 0"
    for a, b in zip(image_only + gin + [t for t in gw if t is not None], gin + again_in + [t for t in again_w if t is not None]):
        np.testing.assert_array_equal(bits(a), bits(b))      # with or without weight gradients, and call after call


@pytest.mark.parametrize("n", [4100, 4099])
def test_var_scan_signal_and_its_gradients(n):
    """var_scan_signal(...).backward() against the f64 gradients; 4099 is padded to 4100 and sliced back"""
    import torch
    rng = np.random.default_rng(n)
    x = (rng.random(n) * 2 - 1).astype(np.float32)
    w = (rng.random(n) ** 0.25).astype(np.float32)
    g = (rng.random(n) * 2 - 1).astype(np.float32)
    scans = [P0, M0]
    dx = torch.from_numpy(x).cuda().requires_grad_()
    dw = torch.from_numpy(w).cuda().requires_grad_()
    (out,) = rfa.var_scan_signal([dx], [dw], scans)
    assert tuple(out.shape) == (n,)
    out.backward(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    want = reference(rows([x]), rows([w]), scans, np.float64)
    serial = reference(rows([x]), rows([w]), scans, np.float32)
    peak = float(np.max(np.abs(x)))
    err32 = float(np.max(np.abs(serial[0].astype(np.float64) - want[0]))) / peak
    assert_under_bar([out.detach().cpu().numpy()], [want[0][0]], err32, peak, f"var_scan_signal {n}")
    want_in, want_w = loops.backward(rows([x]), rows([w]), scans, rows([g]), np.float64)
    ser_in, ser_w = loops.backward(rows([x]), rows([w]), scans, rows([g]), np.float32)
    grad_cases.assert_under_bar(rows([dx.grad.cpu().numpy()]), want_in, grad_cases.figures(ser_in, want_in)[0], f"var_scan_signal {n} grad_in")
    grad_cases.assert_under_bar(rows([dw.grad.cpu().numpy()]), want_w, grad_cases.figures(ser_w, want_w)[0], f"var_scan_signal {n} grad_w")
    assert float(dw.grad[0]) == 0.0


@pytest.mark.parametrize("zero_phase", [True, False])
def test_smooth_samples(zero_phase):
    """the moving average of an irregularly sampled series: w = exp(-gaps / tau) through the loops; gradients in x and gaps"""
    import torch
    n, tau = 4099, 3.0
    rng = np.random.default_rng(77)
    x = (rng.random((2, n)) * 2 - 1).astype(np.float32)
    gaps = (rng.random(n) ** 2 * 4).astype(np.float32)
    g = (rng.random((2, n)) * 2 - 1).astype(np.float32)
    scans = [P0, M0] if zero_phase else [P0]
    base = float(np.exp(-1.0 / tau))
    dx = torch.from_numpy(x).cuda().requires_grad_()
    dg = torch.from_numpy(gaps).cuda().requires_grad_()
    out = rfa.smooth_samples(dx, dg, tau, zero_phase=zero_phase)
    assert tuple(out.shape) == (2, n)
    out.backward(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    planes = rows([x[0], x[1]])
    want = reference(planes, [np.exp(-gaps.astype(np.float64) / tau)[None, :]], scans, np.float64)
    serial = reference(planes, rows([power_loops.power_weights(gaps, base, np.float32)]), scans, np.float32)
    peak = float(np.max(np.abs(x)))
    err32 = max(float(np.max(np.abs(s.astype(np.float64) - w))) for s, w in zip(serial, want)) / peak
    # (the f64 reference's weights are exp(-gaps / tau) itself: the f32 base and product are part of the yardstick's error)
    assert_under_bar(list(out.detach().cpu().numpy()), [w[0] for w in want], err32, peak, f"smooth_samples zero_phase={zero_phase}")
    grads = rows([g[0], g[1]])
    want_in, want_d = power_loops.power_backward(planes, rows([gaps]), [base], scans, grads, np.float64)
    ser_in, ser_d = power_loops.power_backward(planes, rows([gaps]), [base], scans, grads, np.float32)
    grad_cases.assert_under_bar(rows(list(dx.grad.cpu().numpy())), want_in, grad_cases.figures(ser_in, want_in)[0], "smooth_samples grad_x")
    grad_cases.assert_under_bar(rows([dg.grad.cpu().numpy()]), want_d, grad_cases.figures(ser_d, want_d)[0], "smooth_samples grad_gaps")
    with pytest.raises(rfa.RecFilterError) as e:
        rfa.smooth_samples(dx.detach(), dg.detach(), 1e12)      # the base rounds to 1 in f32: the library's refusal
    assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG


# ---- launch names, argument checks that need a device -----------------------------------------------------------------------------
def test_launch_names_and_execute_refusals():
    import torch
    n = 4100
    x = torch.zeros(n, device="cuda")
    w = torch.full((n,), 0.5, device="cuda")
    with rfa.VarPlan.signal(n, SCAN_LISTS["-x+x"]) as plan:
        _, times = plan.execute_timed([x], [w])
        assert [name for name, _ in times] == ["var_tails_1d", "var_carry_1d", "var_pass2_1d"] * 2
        _, times = plan.execute_power_timed([x], [w], [0.5])
        assert [name for name, _ in times] == ["var_tails_1d", "var_carry_1d", "var_pass2_1d"] * 2
        _, _, times = plan.backward_timed(None, [w], [x])
        assert [name for name, _ in times] == ["var_adj_tails_1d", "var_carry_1d", "var_adj_pass2_1d"] * 2
        _, _, times = plan.backward_timed([x], [w], [x], None, [torch.empty_like(w)])
        forward = ["var_tails_1d", "var_carry_1d", "var_pass2_1d"]
        assert [name for name, _ in times] == forward * 2 + ["var_adj_tails_1d", "var_carry_1d", "var_adj_pass2_1d", "var_grad_x"] * 2
        with pytest.raises(rfa.RecFilterError) as e:
            plan.execute([x], [w], [w])                          # a weight signal that is an output
        assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG
        off = torch.zeros(n + 4, device="cuda")[1:1 + n]         # 4 bytes off a 16-byte boundary
        with pytest.raises(rfa.RecFilterError) as e:
            plan.execute([off], [w])
        assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG


# ---- the C++ front-end ----------------------------------------------------------------------------------------------------------
def test_cpp_frontend_varying_signal(tmp_path):
    """RecFilterVarying(x) on a signal of 12616 samples, both forms and both gradients against loops in the C++ file; compiled here
    with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_varying_signal.cpp")
    exe = str(tmp_path / "test_frontend_varying_signal")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "varying-signal-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
