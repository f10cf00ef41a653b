"""GPU tests of the varying scans on volumes (rf_var_plan_create_volume; VarPlan.volume, var_scan_volume).

Reference: the f64 loops of tests/var_volume_loops.py.  Bar: tests/test_gpu_var_scans.py::assert_under_bar, imported -- max abs
error over the input peak <= max(4 x the f32 serial loop's, 1e-6); gradients under the bar of tests/var_grad_cases.py, per
gradient.  Weight (exponent) volumes hold NaN at element 0 along the axis they are scanned along: column 0 of volume 0 (x), row 0 of
volume 1 (y), slice 0 of volumes 2 and 3 (z).

Three contracts are bit for bit: a volume plan's x / y scans give on every slice what the 2-D VarPlan((H, W)) gives on it; its z
scans give what the 2-D plan's y scans give on the (D, H * W) reshaped volume; a z scan of a depth-1 volume is the identity."""
import ctypes
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import guarded
import recfilter_amd as rfa
import smooth_grad_loops as power_loops
import test_gpu_var_scans as base            # the bar (the module, not its tests)
import var_grad_cases as cases               # the gradients' bar
import var_volume_loops as vloops
from recfilter_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PX, MX, PY, MY, PZ, MZ = (0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1), (2, True, 2), (2, False, 2)
SCAN_LISTS = {"+z": [PZ], "-z": [MZ], "+z-z": [PZ, MZ], "-z+z": [MZ, PZ], "+x-x+y-y+z-z": [PX, MX, PY, MY, PZ, MZ],
              "+z-z two weights": [(2, True, 2), (2, False, 3)]}
# (D, H, W), planes: one tile each way; partial tiles on every axis and a partial wave of z lines (W * H = 4488); 16 z tiles (the
# carry recurrence); three planes; depth 1
SHAPES = [((8, 40, 64), 1), ((70, 66, 68), 1), ((1024, 4, 8), 1), ((3, 130, 132), 3), ((1, 40, 64), 1)]
GRAD_SHAPES = [((70, 66, 68), 1), ((3, 130, 132), 3)]
N_WEIGHTS = 4
BASES = [0.9, 0.98, 0.9, 0.5]
WEIGHT_AXIS = [2, 1, 0, 0]       # the numpy axis volume k is scanned along
AXIS_LETTER = "xyz"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(arrays):
    import torch
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]


def host(tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def poison(volumes):
    for w, axis in zip(volumes, WEIGHT_AXIS):
        index = [slice(None)] * 3
        index[axis] = 0
        w[tuple(index)] = np.nan


@functools.lru_cache(maxsize=None)
def case(shape, planes, form="planes", kind="uniform"):
    """(inputs, weight or exponent volumes) of a shape, seeded; shared by the tests and never written"""
    rng = np.random.default_rng(zlib.crc32(repr((shape, planes, form, kind)).encode()))
    ins = [(rng.random(shape) * 2 - 1).astype(np.float32) for _ in range(planes)]
    if form == "planes":
        ws = [(rng.random(shape) ** 0.25).astype(np.float32) for _ in range(N_WEIGHTS)]       # long memories: mean 0.8
    else:
        ws = [(1.0 + 30.0 * rng.random(shape) ** 4).astype(np.float32) for _ in range(N_WEIGHTS)]
    if kind == "sprinkled":                  # exact 0 and 1 (exponents: +inf and 0), 1 % each
        for w in ws:
            u = rng.random(shape)
            w[u < 0.01] = 0.0 if form == "planes" else np.inf
            w[u > 0.99] = 1.0 if form == "planes" else 0.0
    poison(ws)
    for a in ins + ws:
        a.setflags(write=False)
    return ins, ws


def weights_as(ws, form, dtype):
    if form == "planes":
        return [np.asarray(w, dtype=dtype) for w in ws]
    return vloops.power_weights(ws, BASES, dtype)


@functools.lru_cache(maxsize=None)
def expected(shape, planes, name, form="planes", kind="uniform"):
    """(f64 reference, err / peak of the f32 serial loops, input peak)"""
    ins, ws = case(shape, planes, form, kind)
    want = vloops.reference(ins, weights_as(ws, form, np.float64), SCAN_LISTS[name], np.float64)
    serial = vloops.reference(ins, weights_as(ws, form, np.float32), SCAN_LISTS[name], np.float32)
    peak = max(float(np.max(np.abs(p))) for p in ins)
    err32 = max(float(np.max(np.abs(s.astype(np.float64) - w))) for s, w in zip(serial, want)) / peak
    return want, err32, peak


def execute(plan, src, ws, form, outs=None):
    return plan.execute(src, ws, outs) if form == "planes" else plan.execute_power(src, ws, BASES[:plan.n_weights], outs)


def run(shape, planes, scans, ins, ws, form="planes", inplace=False):
    with rfa.VarPlan.volume(shape, scans, planes=planes, n_weights=N_WEIGHTS) as plan:
        src = dev(ins)
        return host(execute(plan, src, dev(ws), form, src if inplace else None))


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["planes", "power"])
@pytest.mark.parametrize("name", list(SCAN_LISTS))
@pytest.mark.parametrize("shape,planes", SHAPES)
def test_against_f64_loops(shape, planes, name, form):
    ins, ws = case(shape, planes, form)
    want, err32, peak = expected(shape, planes, name, form)
    got = run(shape, planes, SCAN_LISTS[name], ins, ws, form)
    base.assert_under_bar(got, want, err32, peak, f"{form} {shape} x {planes} {name}")


@pytest.mark.parametrize("form", ["planes", "power"])
@pytest.mark.parametrize("name", ["+z", "-z", "+z-z", "+x-x+y-y+z-z"])
def test_weights_with_exact_zeros_and_ones(name, form):
    shape, planes = (70, 66, 68), 1
    ins, ws = case(shape, planes, form, "sprinkled")
    assert (ws[2] == 0).any() and ((ws[2] == 1).any() or np.isinf(ws[2]).any())
    want, err32, peak = expected(shape, planes, name, form, "sprinkled")
    base.assert_under_bar(run(shape, planes, SCAN_LISTS[name], ins, ws, form), want, err32, peak, f"sprinkled {form} {name}")


@pytest.mark.parametrize("form", ["planes", "power"])
@pytest.mark.parametrize("name", ["+z", "-z", "+z-z", "-z+z", "+z-z two weights"])
def test_a_z_scan_of_depth_one_is_the_identity(name, form):
    shape = (1, 40, 64)
    ins, ws = case(shape, 1, form)
    got = run(shape, 1, SCAN_LISTS[name], ins, ws, form)
    np.testing.assert_array_equal(bits(got[0]), bits(ins[0]))


# ---- the container does not matter: bit for bit ---------------------------------------------------------------------------------
def backward(plan, ins, ws, g, form, with_weights, used):
    import torch
    gw = [torch.full_like(w, 7.0) if k in used else None for k, w in enumerate(ws)] if with_weights else None
    if form == "planes":
        gin, gw = plan.backward(ins, ws, g, None, gw)
    else:
        gin, gw = plan.backward_power(ins, ws, BASES[:plan.n_weights], g, None, gw)
    torch.cuda.synchronize()
    return gin, gw


@functools.lru_cache(maxsize=None)
def grad_out(shape, planes):
    rng = np.random.default_rng(zlib.crc32(repr(("grad_out", shape, planes)).encode()))
    g = [(rng.random(shape) * 2 - 1).astype(np.float32) for _ in range(planes)]
    for a in g:
        a.setflags(write=False)
    return g


@pytest.mark.parametrize("form", ["planes", "power"])
@pytest.mark.parametrize("scans", [[PX, MX, PY, MY], [MX, PY, PX]], ids=["+x-x+y-y", "-x+y+x"])
@pytest.mark.parametrize("shape,planes", GRAD_SHAPES)
def test_x_and_y_scans_equal_the_image_plan_on_every_slice(shape, planes, scans, form):
    import torch
    D, H, W = shape
    ins, ws = (dev(a) for a in case(shape, planes, form))
    g = dev(grad_out(shape, planes))
    with rfa.VarPlan.volume(shape, scans, planes=planes, n_weights=N_WEIGHTS) as vol, \
            rfa.VarPlan((H, W), scans, planes=planes, n_weights=N_WEIGHTS) as img:
        out = execute(vol, ins, ws, form)
        gin, gw = backward(vol, ins, ws, g, form, True, {0, 1})
        gin_only, _ = backward(vol, ins, ws, g, form, False, {0, 1})
        for z in range(D):
            at = lambda ts: [t[z] if t is not None else None for t in ts]      # noqa: E731
            want = execute(img, at(ins), at(ws), form)
            want_gin, want_gw = backward(img, at(ins), at(ws), at(g), form, True, {0, 1})
            for a, b in zip(at(out) + at(gin) + at(gin_only) + at(gw[:2]), want + want_gin + want_gin + want_gw[:2]):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"slice {z}"


@pytest.mark.parametrize("form", ["planes", "power"])
@pytest.mark.parametrize("name", ["+z-z", "-z+z", "+z-z two weights"])
@pytest.mark.parametrize("shape,planes", GRAD_SHAPES + [((1024, 4, 8), 1)])
def test_z_scans_equal_the_y_scans_of_the_reshaped_image(shape, planes, name, form):
    import torch
    D, H, W = shape
    scans = SCAN_LISTS[name]
    as_y = [(1, causal, k) for _, causal, k in scans]
    used = {k for _, _, k in scans}
    ins, ws = (dev(a) for a in case(shape, planes, form))
    g = dev(grad_out(shape, planes))
    flat = lambda ts: [t.view(D, H * W) if t is not None else None for t in ts]      # noqa: E731
    with rfa.VarPlan.volume(shape, scans, planes=planes, n_weights=N_WEIGHTS) as vol, \
            rfa.VarPlan((D, H * W), as_y, planes=planes, n_weights=N_WEIGHTS) as img:
        out = execute(vol, ins, ws, form)
        gin, gw = backward(vol, ins, ws, g, form, True, used)
        want = execute(img, flat(ins), flat(ws), form)
        want_gin, want_gw = backward(img, flat(ins), flat(ws), flat(g), form, True, used)
        for a, b in zip(flat(out) + flat(gin) + [t for t in flat(gw) if t is not None], want + want_gin + [t for t in want_gw if t is not None]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("form", ["planes", "power"])
@pytest.mark.parametrize("shape,planes", GRAD_SHAPES)
def test_in_place_equals_out_of_place(shape, planes, form):
    ins, ws = case(shape, planes, form)
    scans = SCAN_LISTS["+x-x+y-y+z-z"]
    a, b = run(shape, planes, scans, ins, ws, form), run(shape, planes, scans, ins, ws, form, inplace=True)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(bits(x), bits(y))


def test_a_plan_keeps_no_state():
    """three executes of one plan, a NaN volume in between: the first and the third agree bit for bit"""
    import torch
    shape, planes = (70, 66, 68), 1
    ins, ws = (dev(a) for a in case(shape, planes))
    with rfa.VarPlan.volume(shape, SCAN_LISTS["+x-x+y-y+z-z"], planes=planes, n_weights=N_WEIGHTS) as plan:
        first = host(plan.execute(ins, ws))
        nan = host(plan.execute([torch.full_like(ins[0], float("nan"))], ws))
        third = host(plan.execute(ins, ws))
    assert np.isnan(nan[0]).all()
    np.testing.assert_array_equal(bits(first[0]), bits(third[0]))


def constant_weights(shape, value):
    ws = [np.full(shape, value, dtype=np.float32) for _ in range(N_WEIGHTS)]
    poison(ws)
    return ws


def test_weights_of_zero_return_the_volume():
    shape = (70, 66, 68)
    ins, _ = case(shape, 1)
    for name in SCAN_LISTS:
        got = run(shape, 1, SCAN_LISTS[name], ins, constant_weights(shape, 0.0))
        np.testing.assert_array_equal(bits(got[0]), bits(ins[0]), err_msg=name)


def test_weights_of_one_along_z_spread_slice_zero():
    shape = (70, 66, 68)
    ins, _ = case(shape, 1)
    for name in ("+z", "+z-z"):
        got = run(shape, 1, SCAN_LISTS[name], ins, constant_weights(shape, 1.0))
        np.testing.assert_array_equal(got[0], np.broadcast_to(ins[0][:1], shape), err_msg=name)
    got = run(shape, 1, SCAN_LISTS["-z"], ins, constant_weights(shape, 1.0))
    np.testing.assert_array_equal(got[0], np.broadcast_to(ins[0][-1:], shape))


# ---- guarded volumes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,planes", GRAD_SHAPES)
def test_guarded_volumes(shape, planes):
    import torch
    ins, ws = case(shape, planes)
    g = grad_out(shape, planes)
    name = "+x-x+y-y+z-z"
    d_in, g_in = guarded.guarded_planes(shape, np.float32, planes, fill=guarded.IN_FILL)
    d_w, g_w = guarded.guarded_planes(shape, np.float32, N_WEIGHTS, fill=guarded.IN_FILL)
    d_g, g_g = guarded.guarded_planes(shape, np.float32, planes, fill=guarded.IN_FILL)
    d_out, g_out = guarded.guarded_planes(shape, np.float32, planes, fill=guarded.OUT_FILL)
    d_gin, g_gin = guarded.guarded_planes(shape, np.float32, planes, fill=guarded.OUT_FILL)
    d_gw, g_gw = guarded.guarded_planes(shape, np.float32, 3, fill=guarded.OUT_FILL)
    for checker, arrays in ((g_in, ins), (g_w, ws), (g_g, g)):
        checker.load([torch.from_numpy(np.array(a)) for a in arrays])
        checker.snapshot()
    with rfa.VarPlan.volume(shape, SCAN_LISTS[name], planes=planes, n_weights=N_WEIGHTS) as plan:
        plan.execute(d_in, d_w, d_out)
        plan.backward(d_in, d_w, d_g, d_gin, d_gw + [None])
        torch.cuda.synchronize()
    for checker, what in ((g_out, "output"), (g_gin, "grad_in"), (g_gw, "weight gradients")):
        checker.check_guards(what)
    for checker, what in ((g_in, "input"), (g_w, "weights"), (g_g, "grad_out")):
        checker.check_unchanged(what)
    want, err32, peak = expected(shape, planes, name)
    base.assert_under_bar(host(d_out), want, err32, peak, f"guarded {shape} x {planes}")


# ---- gradients ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_gradients(shape, planes, name, form):
    """f64 gradients and the f32 serial loops' figures: (grad_ins, grad_weights, err32 of grad_ins, [err32 per weight volume])"""
    ins, ws = case(shape, planes, form)
    g = grad_out(shape, planes)
    if form == "planes":
        want_in, want_w = vloops.backward(ins, ws, SCAN_LISTS[name], g, np.float64)
        ser_in, ser_w = vloops.backward(ins, ws, SCAN_LISTS[name], g, np.float32)
    else:
        want_in, want_w = vloops.power_backward(ins, ws, BASES, SCAN_LISTS[name], g, np.float64)
        ser_in, ser_w = vloops.power_backward(ins, ws, BASES, SCAN_LISTS[name], g, np.float32)
    err_w = [None if w is None else cases.figures([s], [w])[0] for s, w in zip(ser_w, want_w)]
    return want_in, want_w, cases.figures(ser_in, want_in)[0], err_w


@pytest.mark.parametrize("form", ["planes", "power"])
@pytest.mark.parametrize("name", ["+z-z", "-z+z", "+x-x+y-y+z-z", "+z-z two weights"])
@pytest.mark.parametrize("shape,planes", GRAD_SHAPES)
def test_gradients_against_f64_loops(shape, planes, name, form):
    scans = SCAN_LISTS[name]
    used = {k for _, _, k in scans}
    ins, ws = (dev(a) for a in case(shape, planes, form))
    g = dev(grad_out(shape, planes))
    with rfa.VarPlan.volume(shape, scans, planes=planes, n_weights=N_WEIGHTS) as plan:
        gin, gw = backward(plan, ins, ws, g, form, True, used)
        again_in, again_w = backward(plan, ins, ws, g, form, True, used)
        only_in, none = backward(plan, ins, ws, g, form, False, used)
    assert none is None
    gin, again_in, only_in = host(gin), host(again_in), host(only_in)
    want_in, want_w, err_in, err_w = expected_gradients(shape, planes, name, form)
    what = f"{form} {shape} x {planes} {name}"
    cases.assert_under_bar(gin, want_in, err_in, f"{what} grad_in")
    for a, b, c in zip(gin, again_in, only_in):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg="call after call")
        np.testing.assert_array_equal(bits(a), bits(c), err_msg="with and without weight gradients")
    for k in sorted(used):
        got, again = gw[k].cpu().numpy(), again_w[k].cpu().numpy()
        cases.assert_under_bar([got], [want_w[k]], err_w[k], f"{what} grad_w[{k}]")
        np.testing.assert_array_equal(bits(got), bits(again), err_msg="call after call")
        first = np.take(got, 0, axis=WEIGHT_AXIS[k])
        assert np.array_equal(bits(first), np.zeros(first.shape, dtype=np.uint32)), f"{what} grad_w[{k}]: element 0 is not exactly +0"


def test_var_scan_volume_and_its_gradients():
    import torch
    shape, planes, name = (70, 66, 68), 1, "+x-x+y-y+z-z"
    ins, ws = case(shape, planes)
    x = dev(ins)[0].requires_grad_(True)
    weights = [w.requires_grad_(k < 3) for k, w in enumerate(dev(ws))]
    out = rfa.var_scan_volume([x], weights, SCAN_LISTS[name])
    want, err32, peak = expected(shape, planes, name)
    base.assert_under_bar(host([o.detach() for o in out]), want, err32, peak, "var_scan_volume")
    g = dev(grad_out(shape, planes))[0]
    (out[0] * g).sum().backward()
    want_in, want_w, err_in, err_w = expected_gradients(shape, planes, name, "planes")
    cases.assert_under_bar(host([x.grad]), want_in, err_in, "var_scan_volume grad_in")
    for k in range(3):
        cases.assert_under_bar(host([weights[k].grad]), [want_w[k]], err_w[k], f"var_scan_volume grad_w[{k}]")
    assert weights[3].grad is None


# ---- launches and refusals ------------------------------------------------------------------------------------------------------
def test_timed_calls_name_the_launches():
    shape, planes = (8, 40, 64), 1
    ins, ws = (dev(a) for a in case(shape, planes))
    g = dev(grad_out(shape, planes))
    stage = lambda prefix, a: [f"{prefix}tails_{a}", "var_carry", f"{prefix}pass2_{a}"]      # noqa: E731
    with rfa.VarPlan.volume(shape, SCAN_LISTS["+x-x+y-y+z-z"], planes=planes, n_weights=N_WEIGHTS) as plan:
        _, report = plan.execute_timed(ins, ws)
        assert [n for n, _ in report] == stage("var_", "x") + stage("var_", "y") + stage("var_", "z")
        _, report = plan.execute_power_timed(ins, ws, BASES)
        assert [n for n, _ in report] == stage("var_", "x") + stage("var_", "y") + stage("var_", "z")
        assert all(ms > 0 for _, ms in report)
        _, _, report = plan.backward_timed(None, ws, g)
        assert [n for n, _ in report] == sum((stage("var_adj_", a) for a in "zzyyxx"), [])
        import torch
        gw = [torch.empty_like(w) for w in ws[:3]] + [None]
        _, _, report = plan.backward_power_timed(ins, ws, BASES, g, None, gw)
        names = [n for n, _ in report]
        assert names[:18] == sum((stage("var_", a) for a in "xxyyzz"), [])
        assert names[18:] == sum((stage("var_adj_", a) + [f"var_grad_{a}"] for a in "zzyyxx"), [])


def test_execute_refusals():
    import torch
    shape = (8, 40, 64)
    ins, ws = (dev(a) for a in case(shape, 1))
    with rfa.VarPlan.volume(shape, [PZ, MZ], planes=1, n_weights=N_WEIGHTS) as plan:
        raw = torch.zeros(int(np.prod(shape)) + 4, dtype=torch.float32, device="cuda")
        misaligned = raw[1:1 + int(np.prod(shape))].view(shape)
        with pytest.raises(rfa.RecFilterError) as e:
            plan.execute([misaligned], ws)
        assert e.value.status == capi.RF_ERR_INVALID_ARG and "aligned" in str(e.value)
        with pytest.raises(rfa.RecFilterError) as e:
            plan.execute(ins, ws, [ws[2]])
        assert e.value.status == capi.RF_ERR_INVALID_ARG and "overlaps" in str(e.value)
        # the last slice of a weight volume is part of it: an output that begins there is refused too
        tail = torch.zeros(2 * int(np.prod(shape)), dtype=torch.float32, device="cuda")
        w_tail, out_tail = tail[:int(np.prod(shape))].view(shape), tail[int(np.prod(shape)) - 40 * 64:][:int(np.prod(shape))].view(shape)
        with pytest.raises(rfa.RecFilterError) as e:
            plan.execute(ins, ws[:2] + [w_tail, ws[3]], [out_tail])
        assert e.value.status == capi.RF_ERR_INVALID_ARG and "overlaps" in str(e.value)


def test_cpp_frontend_varying_volume(tmp_path):
    """RecFilterVarying(x, y, z) in both forms with both gradients and RecFilterSmooth on a volume, against loops in the C++ file;
    compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_varying_volume.cpp")
    exe = str(tmp_path / "test_frontend_varying_volume")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "varying-volume-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
