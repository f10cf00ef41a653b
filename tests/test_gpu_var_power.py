"""GPU tests of the power form of the spatially varying scans (rf_var_plan_execute_power: the weight planes hold exponents d,
the kernels form w = exp2(d * log2(base))) and of rf_var_distances (the two exponent planes of the domain-transform filter).

The scans.  Truth: the f64 serial loops of tests/test_gpu_var_scans.py fed 2^(d * log2(base)) in f64, `base` taken as the f32
value passed in.  Yardstick: the numpy f32 serial loop fed np.exp2(d * np.float32(log2 base)) in f32.  Bar: the project's own,
max abs error over the input peak <= max(4 x the yardstick's, 1e-6).  Exponent planes are 1 + 30 u^4 for seeded uniform u with
NaN at element 0 of the scanned dimension; inputs are those of tests/test_gpu_var_scans.py.

The distances.  Against the f64 formula, per element |got - want| <= (C + 3) * 2^-23 * want: the exact count is one rounding
per difference, C - 1 additions, one multiply and one add, all on non-negative terms, (C + 2) * 2^-24; the bound doubles that
and adds one."""
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
import test_gpu_var_scans as base            # the serial loops, the shapes, the scan lists and the bar (the module, not its tests)
from recfilter_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCAN_LISTS, SHAPES = base.SCAN_LISTS, base.SHAPES
# (base of exponent plane 0, the x scans'; of plane 1, the y scans')
BASES = [(0.5, 0.5), (0.9, 0.9), (0.98, 0.98), (0.5, 0.98)]


# ---- the conversion, as the header states it --------------------------------------------------------------------------------
def weights_f64(d, b):
    with np.errstate(invalid="ignore"):
        return np.exp2(d.astype(np.float64) * np.log2(np.float64(np.float32(b))))


def weights_f32(d, b):
    with np.errstate(invalid="ignore"):
        w = np.exp2(d * np.float32(np.log2(np.float64(np.float32(b)))))
    assert w.dtype == np.float32
    return w


@functools.lru_cache(maxsize=None)
def exponents(shape, kind="uniform"):
    """[d_x, d_y] of a shape, seeded; shared by the tests and never written"""
    rng = np.random.default_rng(zlib.crc32(repr((shape, kind, "exponents")).encode()))
    ds = [(1.0 + 30.0 * rng.random(shape) ** 4).astype(np.float32) for _ in range(2)]
    if kind == "sprinkled":                                   # exponents of exactly 0 (w = 1) and +inf (w = 0), 1 % each
        for d in ds:
            u = rng.random(shape)
            d[u < 0.01] = 0.0
            d[u > 0.99] = np.inf
    base.poison_element_zero(*ds)
    for d in ds:
        d.setflags(write=False)
    return ds


@functools.lru_cache(maxsize=None)
def expected(shape, planes, name, bases, kind="uniform"):
    """(f64 truth, err / peak of the f32 yardstick, input peak)"""
    ins, _ = base.case(shape, planes)
    ds = exponents(shape, kind)
    want = base.reference(ins, [weights_f64(d, b) for d, b in zip(ds, bases)], SCAN_LISTS[name], np.float64)
    serial = base.reference(ins, [weights_f32(d, b) for d, b in zip(ds, bases)], SCAN_LISTS[name], np.float32)
    peak = max(float(np.max(np.abs(p))) for p in ins)
    err32 = max(float(np.max(np.abs(s.astype(np.float64) - w))) for s, w in zip(serial, want)) / peak
    return want, err32, peak


def run_power(shape, planes, scans, ins, ds, bases, inplace=False):
    import torch
    with rfa.VarPlan(shape, scans, planes=planes, n_weights=2) as plan:
        src = base.to_device(ins)
        outs = plan.execute_power(src, base.to_device(ds), list(bases), src if inplace else None)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]


# ---- accuracy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bases", BASES, ids=lambda b: f"a{b[0]}-{b[1]}")
@pytest.mark.parametrize("name", list(SCAN_LISTS))
@pytest.mark.parametrize("shape,planes", SHAPES)
def test_against_f64_loops(shape, planes, name, bases):
    ins, _ = base.case(shape, planes)
    want, err32, peak = expected(shape, planes, name, bases)
    got = run_power(shape, planes, SCAN_LISTS[name], ins, exponents(shape), bases)
    base.assert_under_bar(got, want, err32, peak, f"power {shape} x {planes} {name} bases {bases}")


# ---- exact cases ------------------------------------------------------------------------------------------------------------
EXACT_SHAPE = base.EXACT_SHAPE


def constant_exponents(value):
    ds = [np.full(EXACT_SHAPE, value, dtype=np.float32) for _ in range(2)]
    base.poison_element_zero(*ds)
    return ds


@pytest.mark.parametrize("bases", [(0.5, 0.5), (0.98, 0.9)], ids=str)
@pytest.mark.parametrize("name,dim,sample", [("+x", 0, "first"), ("-x", 0, "last"), ("+x-x", 0, "first"),
                                             ("+y", 1, "first"), ("-y", 1, "last"), ("+y-y", 1, "first")])
def test_exponents_of_zero_spread_one_sample(name, dim, sample, bases):
    """d = 0 is w = 1 exactly, whatever the base: every line equals its first (last) sample"""
    ins, _ = base.case(EXACT_SHAPE, 1)
    got = run_power(EXACT_SHAPE, 1, SCAN_LISTS[name], ins, constant_exponents(0.0), bases)[0]
    x = ins[0]
    if dim == 0:
        want = np.repeat(x[:, :1] if sample == "first" else x[:, -1:], x.shape[1], axis=1)
    else:
        want = np.repeat(x[:1, :] if sample == "first" else x[-1:, :], x.shape[0], axis=0)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("bases", [(0.5, 0.5), (0.98, 0.9)], ids=str)
def test_exponents_of_infinity_leave_the_image(bases):
    """d = +inf is w = 0 exactly: out == in, bit for bit"""
    ins, _ = base.case(EXACT_SHAPE, 1)
    for name in ("+x", "-x", "+y", "-y", "+x-x", "+y-y", "+x-x+y-y"):
        got = run_power(EXACT_SHAPE, 1, SCAN_LISTS[name], ins, constant_exponents(np.inf), bases)
        np.testing.assert_array_equal(got[0].view(np.uint32), ins[0].view(np.uint32), err_msg=name)


@pytest.mark.parametrize("name", ["+x-x", "+y-y", "+x-x+y-y"])
def test_exponents_with_zeros_and_infinities(name):
    shape, planes, bases = EXACT_SHAPE, 1, (0.9, 0.9)
    ins, _ = base.case(shape, planes)
    ds = exponents(shape, "sprinkled")
    assert (ds[0] == 0).any() and np.isinf(ds[0]).any()
    want, err32, peak = expected(shape, planes, name, bases, "sprinkled")
    base.assert_under_bar(run_power(shape, planes, SCAN_LISTS[name], ins, ds, bases), want, err32, peak, f"power sprinkled {name}")


def test_nan_at_element_zero_reaches_nothing():
    ins, _ = base.case(EXACT_SHAPE, 1)
    ds = exponents(EXACT_SHAPE)
    assert np.isnan(ds[0][:, 0]).all() and np.isnan(ds[1][0, :]).all()
    for name in SCAN_LISTS:
        got = run_power(EXACT_SHAPE, 1, SCAN_LISTS[name], ins, ds, (0.9, 0.9))
        assert not np.isnan(got[0]).any(), name


# ---- plan behaviour ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,planes", [((70, 260), 1), ((130, 132), 3)])
def test_in_place_equals_out_of_place(shape, planes):
    ins, _ = base.case(shape, planes)
    scans, ds, bases = SCAN_LISTS["+x-x+y-y"], exponents(shape), (0.9, 0.98)
    a = run_power(shape, planes, scans, ins, ds, bases)
    b = run_power(shape, planes, scans, ins, ds, bases, inplace=True)
    for p, q in zip(a, b):
        np.testing.assert_array_equal(p.view(np.uint32), q.view(np.uint32))


def test_one_plan_runs_either_form_and_keeps_no_state():
    import torch
    shape, planes = (70, 260), 1
    ins, ws = base.case(shape, planes)
    ds, bases = exponents(shape), [0.9, 0.5]
    scans = SCAN_LISTS["+x-x+y-y"]
    fresh_power = run_power(shape, planes, scans, ins, ds, bases)
    with rfa.VarPlan(shape, scans, planes=planes, n_weights=2) as plan:
        dws, dds = base.to_device(ws), base.to_device(ds)
        first = plan.execute(base.to_device(ins), dws)
        power = plan.execute_power(base.to_device(ins), dds, bases)
        third = plan.execute(base.to_device(ins), dws)
        power_again = plan.execute_power(base.to_device(ins), dds, bases)
        torch.cuda.synchronize()
        guarded.assert_bits_equal([t.cpu() for t in third], [t.cpu() for t in first], "execute after execute_power")
        guarded.assert_bits_equal([t.cpu() for t in power_again], [t.cpu() for t in power], "execute_power after execute")
        np.testing.assert_array_equal(power[0].cpu().numpy().view(np.uint32), fresh_power[0].view(np.uint32))
        assert not guarded.bits_equal(power[0].cpu(), first[0].cpu()), "the two forms ran on different weights"


@pytest.mark.parametrize("name", ["+x", "-y", "+x-x+y-y"])
def test_timed_names_the_same_launches(name):
    import torch
    shape = (40, 64)
    ins, ws = base.case(shape, 1)
    with rfa.VarPlan(shape, SCAN_LISTS[name], n_weights=2) as plan:
        _, plain = plan.execute_timed(base.to_device(ins), base.to_device(ws))
        outs, power = plan.execute_power_timed(base.to_device(ins), base.to_device(exponents(shape)), [0.9, 0.9])
        torch.cuda.synchronize()
        assert [n for n, _ in power] == [n for n, _ in plain] and len(power) == plan.num_kernels
        want, err32, peak = expected(shape, 1, name, (0.9, 0.9))
        base.assert_under_bar([o.cpu().numpy() for o in outs], want, err32, peak, f"execute_power_timed {name}")


def test_execute_power_refusals_on_a_device_plan():
    import torch
    shape = (40, 64)
    x = torch.zeros(shape, device="cuda")
    d = torch.ones(shape, device="cuda")
    with rfa.VarPlan(shape, [base.PX]) as plan:
        for bad in (0.0, 1.0, 1.5, float("nan"), -0.5):
            with pytest.raises(rfa.RecFilterError) as e:
                plan.execute_power([x], [d], [bad])
            assert e.value.status == capi.RF_ERR_INVALID_ARG and "plane 0" in str(e.value)
        with pytest.raises(rfa.RecFilterError) as e:
            plan.execute_power([x], [d], [0.5], [d])             # an exponent plane that is an output plane
        assert e.value.status == capi.RF_ERR_INVALID_ARG


# ---- guarded planes ---------------------------------------------------------------------------------------------------------
GUARDED = [((70, 260), 1), ((130, 132), 3)]


@pytest.mark.parametrize("shape,planes", GUARDED)
def test_guarded_planes_power(shape, planes):
    import torch
    ins, _ = base.case(shape, planes)
    ds, bases = exponents(shape), (0.9, 0.98)
    want, err32, peak = expected(shape, planes, "+x-x+y-y", bases)
    d_in, g_in = guarded.guarded_planes(shape, np.float32, planes, fill=guarded.IN_FILL)
    d_d, g_d = guarded.guarded_planes(shape, np.float32, 2, fill=guarded.IN_FILL)
    d_out, g_out = guarded.guarded_planes(shape, np.float32, planes, fill=guarded.OUT_FILL)
    g_in.load([torch.from_numpy(np.array(a)) for a in ins])
    g_d.load([torch.from_numpy(np.array(a)) for a in ds])
    g_in.snapshot()
    g_d.snapshot()
    with rfa.VarPlan(shape, SCAN_LISTS["+x-x+y-y"], planes=planes, n_weights=2) as plan:
        plan.execute_power(d_in, d_d, list(bases), d_out)
        torch.cuda.synchronize()
    g_out.check_guards("output")
    g_in.check_unchanged("input")
    g_d.check_unchanged("exponents")
    base.assert_under_bar([o.cpu().numpy() for o in d_out], want, err32, peak, f"guarded power {shape} x {planes}")


# ---- rf_var_distances -------------------------------------------------------------------------------------------------------
DIST_SHAPES = [(40, 64), (70, 260), (1, 8), (5, 4), (130, 132)]
SCALE = 80.0                  # sigma_s 40 over sigma_r 0.5: exact in f32


@functools.lru_cache(maxsize=None)
def guide_of(shape, channels, kind):
    rng = np.random.default_rng(zlib.crc32(repr((shape, channels, kind, "guide")).encode()))
    if kind == "u8":
        g = rng.integers(0, 256, size=(channels,) + shape, dtype=np.uint8)
    else:
        g = rng.random((channels,) + shape).astype(np.float32)
    g.setflags(write=False)
    return g


def distances_f64(g, scale):
    """the formula of include/recfilter_amd.h in f64 on a (C, H, W) guide"""
    g = g.astype(np.float64)
    dx = np.ones(g.shape[1:])
    dy = np.ones(g.shape[1:])
    dx[:, 1:] += scale * np.abs(g[:, :, 1:] - g[:, :, :-1]).sum(0)
    dy[1:, :] += scale * np.abs(g[:, 1:, :] - g[:, :-1, :]).sum(0)
    return dx, dy


def assert_distances(got, want, channels, what):
    bound = (channels + 3) * 2.0 ** -23
    for axis, g, w in zip("xy", got, want):
        assert g.dtype == np.float32 and not np.isnan(g).any(), f"{what}: d_{axis}"
        rel = float(np.max(np.abs(g.astype(np.float64) - w) / w))
        print(f"{what}: d_{axis} max relative error {rel:.3e}, bound {bound:.3e}")
        assert rel <= bound, f"{what}: d_{axis} is {rel:.3e} off, bound {bound:.3e}"
    np.testing.assert_array_equal(got[0][:, 0], np.float32(1))
    np.testing.assert_array_equal(got[1][0, :], np.float32(1))


def raw_distances(planes, u8, shape, scale, dx, dy):
    """rf_var_distances on device tensors (one per guide plane), on torch's current stream"""
    import torch
    arr = (ctypes.c_void_p * len(planes))(*[p.data_ptr() for p in planes])
    capi.check(capi.lib().rf_var_distances(arr, len(planes), int(u8), shape[1], shape[0], scale, dx.data_ptr(), dy.data_ptr(), -1,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("channels", [1, 3, 16])
@pytest.mark.parametrize("shape", DIST_SHAPES)
def test_distances_against_the_f64_formula(shape, channels, kind):
    import torch
    g = guide_of(shape, channels, kind)
    dev = torch.from_numpy(np.array(g)).cuda()
    dx, dy = (torch.full(shape, float("nan"), device="cuda") for _ in range(2))
    raw_distances([dev[c] for c in range(channels)], kind == "u8", shape, SCALE, dx, dy)
    torch.cuda.synchronize()
    assert_distances((dx.cpu().numpy(), dy.cpu().numpy()), distances_f64(g, SCALE), channels, f"distances {shape} x {channels} {kind}")


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", DIST_SHAPES)
def test_python_distances(shape, channels):
    """domain_transform_distances: a uint8 guide means that guide divided by 255; (H, W) guides; f32 guides"""
    import torch
    sigma_s, sigma_r = 40.0, 0.5
    g8 = guide_of(shape, channels, "u8")
    dx, dy = rfa.domain_transform_distances(torch.from_numpy(np.array(g8)).cuda(), sigma_s, sigma_r)
    torch.cuda.synchronize()
    assert_distances((dx.cpu().numpy(), dy.cpu().numpy()), distances_f64(g8.astype(np.float64) / 255.0, sigma_s / sigma_r), channels,
                     f"python distances {shape} x {channels} u8")
    gf = guide_of(shape, channels, "f32")
    dx, dy = rfa.domain_transform_distances(torch.from_numpy(np.array(gf)).cuda(), sigma_s, sigma_r)
    one = rfa.domain_transform_distances(torch.from_numpy(np.array(gf[0])).cuda(), sigma_s, sigma_r)
    torch.cuda.synchronize()
    assert_distances((dx.cpu().numpy(), dy.cpu().numpy()), distances_f64(gf, sigma_s / sigma_r), channels, f"python distances {shape} x {channels} f32")
    assert_distances([t.cpu().numpy() for t in one], distances_f64(gf[:1], sigma_s / sigma_r), 1, f"python distances {shape} (H, W)")


@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("shape,channels", GUARDED)
def test_guarded_planes_distances(shape, channels, kind):
    """Guards of 0xFF around the guide planes (NaN in f32; for bytes a second run with 0x00 guards, bit-identical), guards of
    0xA5 around d_x and d_y"""
    import torch
    g = guide_of(shape, channels, kind)
    dtype = np.uint8 if kind == "u8" else np.float32
    results = []
    for fill in (guarded.IN_FILL, guarded.IN_FILL_ZERO) if kind == "u8" else (guarded.IN_FILL,):
        d_g, g_g = guarded.guarded_planes(shape, dtype, channels, fill=fill)
        d_o, g_o = guarded.guarded_planes(shape, np.float32, 2, fill=guarded.OUT_FILL)
        g_g.load([torch.from_numpy(np.array(g[c])) for c in range(channels)])
        g_g.snapshot()
        raw_distances(d_g, kind == "u8", shape, SCALE, d_o[0], d_o[1])
        torch.cuda.synchronize()
        g_o.check_guards("d_x, d_y")
        g_g.check_unchanged("guide")
        results.append([t.clone().cpu() for t in d_o])
    assert_distances([t.numpy() for t in results[0]], distances_f64(g, SCALE), channels, f"guarded distances {shape} x {channels} {kind}")
    if len(results) == 2:
        guarded.assert_bits_equal(results[1], results[0], "guide guards of 0x00 against 0xFF")


def test_distances_refusals_on_a_device():
    import torch
    shape = (8, 16)
    g = torch.zeros(shape, device="cuda")
    both = torch.zeros((2,) + shape, device="cuda")
    lib = capi.lib()

    def status(planes, dx, dy, u8=0):
        arr = (ctypes.c_void_p * len(planes))(*planes)
        return lib.rf_var_distances(arr, len(planes), u8, shape[1], shape[0], 1.0, dx, dy, -1, None)
    assert status([g.data_ptr()], both[0].data_ptr(), both[0].data_ptr()) == capi.RF_ERR_INVALID_ARG            # dx is dy
    assert status([g.data_ptr()], g.data_ptr(), both[1].data_ptr()) == capi.RF_ERR_INVALID_ARG                  # dx is the guide
    assert status([g.data_ptr()], both[0].data_ptr() + 4, both[1].data_ptr()) == capi.RF_ERR_INVALID_ARG        # alignment
    assert status([g.data_ptr() + 2], both[0].data_ptr(), both[1].data_ptr(), u8=1) == capi.RF_ERR_INVALID_ARG
    assert status([g.data_ptr()], both[0].data_ptr(), both[1].data_ptr()) == capi.RF_OK
    torch.cuda.synchronize()


# ---- the whole filter -------------------------------------------------------------------------------------------------------
def smooth_case():
    C, H, W = 3, 96, 132
    rng = np.random.default_rng(2011)
    step = np.where(np.arange(W) < W // 2, 0.2, 0.8).astype(np.float32)
    clean = np.broadcast_to(step, (C, H, W))
    image = (clean + 0.02 * rng.standard_normal((C, H, W))).astype(np.float32)
    return image, clean


def assert_step_kept_noise_gone(image, clean, got, what):
    W = image.shape[2]
    left, right = slice(8, W // 2 - 8), slice(W // 2 + 8, W - 8)
    contrast_in = image[:, :, W // 2:].mean() - image[:, :, :W // 2].mean()
    contrast_out = got[:, :, W // 2:].mean() - got[:, :, :W // 2].mean()
    noise_in = np.mean([(image - clean)[:, :, s].std() for s in (left, right)])
    noise_out = np.mean([(got - clean)[:, :, s].std() for s in (left, right)])
    print(f"{what}: contrast {contrast_in:.4f} -> {contrast_out:.4f}, flat-side noise {noise_in:.4f} -> {noise_out:.4f}")
    assert contrast_out >= 0.9 * contrast_in, (contrast_out, contrast_in)
    assert noise_out <= 0.5 * noise_in, (noise_out, noise_in)


def test_edge_aware_smooth_power():
    import torch
    image, clean = smooth_case()
    C = image.shape[0]
    sigma_s, sigma_r, K = 40.0, 0.5, 3
    dev = torch.from_numpy(image).cuda()
    got = rfa.edge_aware_smooth(dev, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, form="power")
    dx, dy = rfa.domain_transform_distances(dev, sigma_s, sigma_r)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    # the f64 domain-transform filter fed the distance planes and the bases the library computed
    ds = [dx.cpu().numpy(), dy.cpu().numpy()]
    bases = rfa.domain_transform_bases(sigma_s, K)
    assert len(bases) == K
    want = [image[c].astype(np.float64) for c in range(C)]
    serial = [image[c] for c in range(C)]
    for a_k in bases:
        want = base.reference(want, [weights_f64(d, a_k) for d in ds], SCAN_LISTS["+x-x+y-y"], np.float64)
        serial = base.reference(serial, [weights_f32(d, a_k) for d in ds], SCAN_LISTS["+x-x+y-y"], np.float32)
    peak = float(np.max(np.abs(image)))
    err32 = max(float(np.max(np.abs(s.astype(np.float64) - w))) for s, w in zip(serial, want)) / peak
    base.assert_under_bar(list(got), want, err32, peak, "edge_aware_smooth, power form")
    assert_step_kept_noise_gone(image, clean, got, "edge_aware_smooth, power form")
    # (H, W) images and an explicit guide take the same path
    one = rfa.edge_aware_smooth(dev[0], guide=dev, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, form="power")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(one.cpu().numpy(), got[0])
    # a byte guide built from the image
    g8 = torch.from_numpy(np.rint(255.0 * np.clip(image, 0.0, 1.0)).astype(np.uint8)).cuda()
    bytes_guided = rfa.edge_aware_smooth(dev, guide=g8, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, form="power")
    torch.cuda.synchronize()
    assert_step_kept_noise_gone(image, clean, bytes_guided.cpu().numpy(), "edge_aware_smooth, power form, uint8 guide")


def test_edge_aware_smooth_planes_is_what_it_was():
    """form="planes" (the default): the weight planes of domain_transform_weights, one execute per iteration, bit for bit"""
    import torch
    image, _ = smooth_case()
    C, H, W = image.shape
    sigma_s, sigma_r, K = 40.0, 0.5, 3
    dev = torch.from_numpy(image).cuda()
    default = rfa.edge_aware_smooth(dev, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K)
    planes = rfa.edge_aware_smooth(dev, sigma_s=sigma_s, sigma_r=sigma_r, iterations=K, form="planes")
    src = [dev[c].contiguous() for c in range(C)]
    with rfa.VarPlan((H, W), SCAN_LISTS["+x-x+y-y"], planes=C, n_weights=2) as plan:
        for wx, wy in rfa.domain_transform_weights(dev, sigma_s, sigma_r, K):
            src = plan.execute(src, [wx, wy])
        torch.cuda.synchronize()
    by_hand = [t.cpu() for t in src]
    guarded.assert_bits_equal([planes[c].cpu() for c in range(C)], by_hand, 'form="planes" against the executes written out')
    guarded.assert_bits_equal([default[c].cpu() for c in range(C)], by_hand, "the default form against the executes written out")
    with pytest.raises(ValueError):
        rfa.edge_aware_smooth(dev, form="weights")


# ---- the C++ front-end ------------------------------------------------------------------------------------------------------
def test_cpp_frontend_varying_power(tmp_path):
    """domain_transform_distances, then RecFilterVarying::realize_power with +x -x +y -y on 70 x 260 against loops in the C++
    file, under the bar above; compiled here with the command line of test_cpp_frontend_varying"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_varying_power.cpp")
    exe = str(tmp_path / "test_frontend_varying_power")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "varying-power-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
