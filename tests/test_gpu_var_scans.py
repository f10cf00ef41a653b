"""GPU tests of the spatially varying first-order scans (kernels_var.hip, plan_var.cpp, recfilter_amd/varscan.py).

Reference: the recurrences of include/recfilter_amd.h in numpy f64, written here.  Bar: max abs error over the input peak
<= max(4 x the same figure of the numpy f32 serial loop on that case, 1e-6) -- the factor 4 allows for FMA contraction and the
tiled order of operations.  Weight planes hold NaN at element 0 of the scanned dimension unless a test says otherwise; inputs
are seeded, signed, in [-1, 1]."""
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import guarded
import recfilter_amd as rfa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# x scans take weight plane 0 (NaN in column 0), y scans weight plane 1 (NaN in row 0)
PX, MX, PY, MY = (0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1)
SCAN_LISTS = {"+x": [PX], "-x": [MX], "+x-x": [PX, MX], "+y": [PY], "-y": [MY], "+y-y": [PY, MY], "+x-x+y-y": [PX, MX, PY, MY]}
# (H, W), planes: one tile each way; a partial tile each way over two or more tiles; 16 tiles along x with a partial row tile;
# 16 tiles along y with a 2-chunk width; three planes
SHAPES = [((40, 64), 1), ((70, 260), 1), ((8, 1024), 1), ((1024, 8), 1), ((130, 132), 3)]


# ---- the reference: serial loops ----------------------------------------------------------------------------------------------
def scan_lines(v, w, causal):
    """one scan along axis 1 of v (lines, N) in v's type; w[:, 0] is never read"""
    n = v.shape[1]
    one = v.dtype.type(1)
    wt = np.zeros((v.shape[0], n + 1), dtype=v.dtype)
    wt[:, 1:n] = w[:, 1:n]
    y = np.empty_like(v)
    acc = np.zeros(v.shape[0], dtype=v.dtype)
    order = range(n) if causal else range(n - 1, -1, -1)
    for i in order:
        wi = wt[:, i] if causal else wt[:, i + 1]
        acc = (one - wi) * v[:, i] + wi * acc
        y[:, i] = acc
    return y


def reference(planes, weights, scans, dtype):
    out = []
    for p in planes:
        v = np.asarray(p, dtype=dtype)
        for dim, causal, k in scans:
            w = np.asarray(weights[k])
            v = scan_lines(v, w, causal) if dim == 0 else np.ascontiguousarray(scan_lines(v.T, w.T, causal).T)
        out.append(v)
    return out


def poison_element_zero(wx, wy):
    wx[:, 0] = np.nan
    wy[0, :] = np.nan


@functools.lru_cache(maxsize=None)
def case(shape, planes, kind="uniform"):
    """(inputs, [wx, wy]) of a shape, seeded; shared by the tests and never written"""
    rng = np.random.default_rng(zlib.crc32(repr((shape, planes, kind)).encode()))
    ins = [(rng.random(shape) * 2 - 1).astype(np.float32) for _ in range(planes)]
    ws = [(rng.random(shape) ** 0.25).astype(np.float32) for _ in range(2)]       # long memories: mean 0.8
    if kind == "sprinkled":                                                       # exact 0 and exact 1, 1 % each
        for w in ws:
            u = rng.random(shape)
            w[u < 0.01] = 0.0
            w[u > 0.99] = 1.0
    poison_element_zero(*ws)
    for a in ins + ws:
        a.setflags(write=False)
    return ins, ws


@functools.lru_cache(maxsize=None)
def expected(shape, planes, name, kind="uniform"):
    """(f64 reference, err / peak of the f32 serial loop, input peak)"""
    ins, ws = case(shape, planes, kind)
    want = reference(ins, ws, SCAN_LISTS[name], np.float64)
    serial = reference(ins, ws, SCAN_LISTS[name], np.float32)
    peak = max(float(np.max(np.abs(p))) for p in ins)
    err32 = max(float(np.max(np.abs(s.astype(np.float64) - w))) for s, w in zip(serial, want)) / peak
    return want, err32, peak


def to_device(arrays):
    import torch
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]


def run(shape, planes, scans, ins, ws, inplace=False):
    import torch
    with rfa.VarPlan(shape, scans, planes=planes, n_weights=2) as plan:
        src = to_device(ins)
        outs = plan.execute(src, to_device(ws), src if inplace else None)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]


def assert_under_bar(got, want, err32, peak, what):
    for g in got:
        assert not np.isnan(g).any(), f"{what}: NaN in the result"
    err = max(float(np.max(np.abs(g.astype(np.float64) - w))) for g, w in zip(got, want)) / peak
    bar = max(4 * err32, 1e-6)
    print(f"{what}: err/peak {err:.3e}, f32 serial loop {err32:.3e}, ratio {err / max(err32, 1e-30):.2f}")
    assert err <= bar, f"{what}: err/peak {err:.3e} above the bar {bar:.3e} (f32 serial loop: {err32:.3e})"


# ---- parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCAN_LISTS))
@pytest.mark.parametrize("shape,planes", SHAPES)
def test_against_f64_loops(shape, planes, name):
    ins, ws = case(shape, planes)
    want, err32, peak = expected(shape, planes, name)
    got = run(shape, planes, SCAN_LISTS[name], ins, ws)
    assert_under_bar(got, want, err32, peak, f"{shape} x {planes} {name}")


@pytest.mark.parametrize("name", ["+x-x", "+y-y", "+x-x+y-y"])
def test_weights_with_exact_zeros_and_ones(name):
    shape, planes = (70, 260), 1
    ins, ws = case(shape, planes, "sprinkled")
    assert (ws[0] == 0).any() and (ws[0] == 1).any()
    want, err32, peak = expected(shape, planes, name, "sprinkled")
    assert_under_bar(run(shape, planes, SCAN_LISTS[name], ins, ws), want, err32, peak, f"sprinkled {name}")


# ---- exact cases: every tile's P, G and carry hand-over -----------------------------------------------------------------------
EXACT_SHAPE = (70, 260)      # 5 tiles along x, 2 along y, the last one partial each way


def constant_weights(value):
    ws = [np.full(EXACT_SHAPE, value, dtype=np.float32) for _ in range(2)]
    poison_element_zero(*ws)
    return ws


def test_weights_of_zero_leave_the_image():
    ins, _ = case(EXACT_SHAPE, 1)
    for name in ("+x", "-x", "+y", "-y", "+x-x+y-y"):
        got = run(EXACT_SHAPE, 1, SCAN_LISTS[name], ins, constant_weights(0.0))
        np.testing.assert_array_equal(got[0], ins[0], err_msg=name)


@pytest.mark.parametrize("name,dim,sample", [("+x", 0, "first"), ("-x", 0, "last"), ("+x-x", 0, "first"),
                                             ("+y", 1, "first"), ("-y", 1, "last"), ("+y-y", 1, "first")])
def test_weights_of_one_spread_one_sample(name, dim, sample):
    ins, _ = case(EXACT_SHAPE, 1)
    got = run(EXACT_SHAPE, 1, SCAN_LISTS[name], ins, constant_weights(1.0))[0]
    x = ins[0]
    if dim == 0:
        want = np.repeat(x[:, :1] if sample == "first" else x[:, -1:], x.shape[1], axis=1)
    else:
        want = np.repeat(x[:1, :] if sample == "first" else x[-1:, :], x.shape[0], axis=0)
    np.testing.assert_array_equal(got, want)


# ---- in place, state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,planes", [((70, 260), 1), ((130, 132), 3)])
def test_in_place_equals_out_of_place(shape, planes):
    ins, ws = case(shape, planes)
    scans = SCAN_LISTS["+x-x+y-y"]
    a = run(shape, planes, scans, ins, ws)
    b = run(shape, planes, scans, ins, ws, inplace=True)
    for p, q in zip(a, b):
        np.testing.assert_array_equal(p.view(np.uint32), q.view(np.uint32))


def test_a_plan_keeps_no_state():
    import torch
    shape, planes = (70, 260), 1
    ins, ws = case(shape, planes)
    other = [np.full(shape, np.nan, dtype=np.float32)]
    scans = SCAN_LISTS["+x-x+y-y"]
    fresh = run(shape, planes, scans, ins, ws)
    with rfa.VarPlan(shape, scans, planes=planes, n_weights=2) as plan:
        dws = to_device(ws)
        results = [plan.execute(to_device(ins), dws) for _ in range(3)]
        plan.execute(to_device(other), dws)                      # a different input in between
        after = plan.execute(to_device(ins), dws)
        torch.cuda.synchronize()
        for r in results[1:] + [after]:
            guarded.assert_bits_equal([t.cpu() for t in r], [t.cpu() for t in results[0]], "repeated executes of one plan")
        np.testing.assert_array_equal(after[0].cpu().numpy().view(np.uint32), fresh[0].view(np.uint32))


# ---- guarded planes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,planes", [((70, 260), 1), ((130, 132), 3)])
def test_guarded_planes(shape, planes):
    import torch
    ins, ws = case(shape, planes)
    want, err32, peak = expected(shape, planes, "+x-x+y-y")
    d_in, g_in = guarded.guarded_planes(shape, np.float32, planes, fill=guarded.IN_FILL)
    d_w, g_w = guarded.guarded_planes(shape, np.float32, 2, fill=guarded.IN_FILL)
    d_out, g_out = guarded.guarded_planes(shape, np.float32, planes, fill=guarded.OUT_FILL)
    g_in.load([torch.from_numpy(np.array(a)) for a in ins])
    g_w.load([torch.from_numpy(np.array(a)) for a in ws])
    g_in.snapshot()
    g_w.snapshot()
    with rfa.VarPlan(shape, SCAN_LISTS["+x-x+y-y"], planes=planes, n_weights=2) as plan:
        plan.execute(d_in, d_w, d_out)
        torch.cuda.synchronize()
    g_out.check_guards("output")
    g_in.check_unchanged("input")
    g_w.check_unchanged("weights")
    assert_under_bar([o.cpu().numpy() for o in d_out], want, err32, peak, f"guarded {shape} x {planes}")


# ---- argument checks that need a device -----------------------------------------------------------------------------------------
def test_execute_refusals():
    import torch
    shape = (40, 64)
    x = torch.zeros(shape, device="cuda")
    w = torch.full(shape, 0.5, device="cuda")
    with rfa.VarPlan(shape, [PX]) as plan:
        with pytest.raises(rfa.RecFilterError) as e:
            plan.execute([x], [w], [w])                          # a weight plane that is an output plane
        assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG
        big = torch.zeros(shape[0] * shape[1] + 4, device="cuda")
        off = big[1:1 + shape[0] * shape[1]].view(shape)         # 4 bytes off a 16-byte boundary
        with pytest.raises(rfa.RecFilterError) as e:
            plan.execute([off], [w])
        assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG
        _, times = plan.execute_timed([x], [w])
        assert [n for n, _ in times] == ["var_tails_x", "var_carry", "var_pass2_x"]


# ---- edge-aware smoothing -------------------------------------------------------------------------------------------------------
def test_edge_aware_smooth():
    import torch
    C, H, W = 3, 96, 132
    rng = np.random.default_rng(2011)
    step = np.where(np.arange(W) < W // 2, 0.2, 0.8).astype(np.float32)
    clean = np.broadcast_to(step, (C, H, W))
    image = (clean + 0.02 * rng.standard_normal((C, H, W))).astype(np.float32)
    sigma_s, sigma_r, K = 40.0, 0.5, 3
    dev = torch.from_numpy(image).cuda()
    weights = rfa.domain_transform_weights(dev, sigma_s, sigma_r, K)
    got = rfa.edge_aware_smooth(dev, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    # the f64 domain-transform filter fed the f32 weight planes the library computed
    assert len(weights) == K and all(w.dtype == torch.float32 and tuple(w.shape) == (H, W) for pair in weights for w in pair)
    want = [image[c].astype(np.float64) for c in range(C)]
    serial = [image[c] for c in range(C)]
    for wx, wy in weights:
        ws = [wx.cpu().numpy(), wy.cpu().numpy()]
        want = reference(want, ws, SCAN_LISTS["+x-x+y-y"], np.float64)
        serial = reference(serial, ws, SCAN_LISTS["+x-x+y-y"], np.float32)
    peak = float(np.max(np.abs(image)))
    err32 = max(float(np.max(np.abs(s.astype(np.float64) - w))) for s, w in zip(serial, want)) / peak
    assert_under_bar(list(got), want, err32, peak, "edge_aware_smooth")
    # the step survives, the noise does not
    left, right = slice(8, W // 2 - 8), slice(W // 2 + 8, W - 8)
    contrast_in = image[:, :, W // 2:].mean() - image[:, :, :W // 2].mean()
    contrast_out = got[:, :, W // 2:].mean() - got[:, :, :W // 2].mean()
    assert contrast_out >= 0.9 * contrast_in, (contrast_out, contrast_in)
    noise_in = np.mean([(image - clean)[:, :, s].std() for s in (left, right)])
    noise_out = np.mean([(got - clean)[:, :, s].std() for s in (left, right)])
    print(f"edge_aware_smooth: contrast {contrast_in:.4f} -> {contrast_out:.4f}, flat-side noise {noise_in:.4f} -> {noise_out:.4f}")
    assert noise_out <= 0.5 * noise_in, (noise_out, noise_in)
    # (H, W) images and an explicit guide take the same path
    one = rfa.edge_aware_smooth(dev[0], guide=dev, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(one.cpu().numpy(), got[0])


# ---- the C++ front-end ----------------------------------------------------------------------------------------------------------
def test_cpp_frontend_varying(tmp_path):
    """RecFilterVarying: +x -x +y -y on 70 x 260 against loops in the C++ file, under the bar above; compiled here with the
    command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_varying.cpp")
    exe = str(tmp_path / "test_frontend_varying")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "varying-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
