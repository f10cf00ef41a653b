"""CPU tests of the bases' gradient of the power form (rf_var_plan_backward_power_bases): the f64 yardstick of
tests/sigma_grad_loops.py against central differences of the f64 filter -- images, a signal, a volume, exponents of +inf and 0
sprinkled in --, the exported surface, and what host-only plans answer: the refusals in their documented order, the launch count
and the workspace.  No kernel is launched."""
import ctypes

import numpy as np
import pytest

import sigma_grad_loops as gloops
import var_grad_cases as vcases
import var_volume_loops as vloops
import recfilter_amd as rfa
from recfilter_amd import capi
from smooth_volume_grad_loops import SCANS as VOLUME_SCANS
from test_smooth_grad_host import H_STEP, TOL      # the step and the tolerance of that file's pins, relative to a peak of >= 1

ALL = vcases.SCAN_LISTS["+x-x+y-y"]
PAIR_1D = [(0, True, 0), (0, False, 0)]


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
def f64_loss(planes, exponents, bases, scans, grad_outs):
    """L = sum(grad_out * out) of the f64 filter with w = base ** d, the bases NOT rounded to f32 (they are stepped by 1e-6)"""
    vols = [gloops.as_volume(np.asarray(p, dtype=np.float64)) for p in planes]
    ws = [np.exp2(gloops.as_volume(np.asarray(d, dtype=np.float64)) * np.log2(np.float64(a))) for d, a in zip(exponents, bases)]
    out = vloops.reference(vols, ws, scans, np.float64)
    return sum(float(np.sum(gloops.as_volume(g) * o)) for g, o in zip(grad_outs, out))


def pin(planes, exponents, bases, scans, grad_outs, what):
    for a in bases:
        assert float(np.float32(a)) == a, "bases the loops' rounding to f32 leaves alone"
    _, got, norms = gloops.power_bases_backward(planes, exponents, bases, scans, grad_outs, np.float64)
    read = {k for _, _, k in scans}
    for k in range(len(bases)):
        up, down = list(bases), list(bases)
        up[k] += H_STEP
        down[k] -= H_STEP
        num = (f64_loss(planes, exponents, up, scans, grad_outs) - f64_loss(planes, exponents, down, scans, grad_outs)) / (2 * H_STEP)
        print(f"sigma_grad_host {what} base {k}: loops {got[k]:.12e}, central differences {num:.12e}, sum|terms| {norms[k]:.3e}")
        assert np.isfinite(got[k]) and abs(num - got[k]) <= TOL * max(1.0, abs(got[k])), (what, k, num, got[k])
        assert (k in read) == (norms[k] > 0), (what, k)
    return got


def exponents_like(shape, rng, n):
    """exponent planes of a guide-like spread: 1 .. 4"""
    return [1.0 + 3.0 * rng.random(shape) for _ in range(n)]


@pytest.mark.parametrize("shape,planes", [((6, 8), 2), ((5, 12), 1)])
def test_f64_base_gradients_of_images_against_central_differences(shape, planes):
    rng = np.random.default_rng(2801)
    ins = [rng.random(shape) * 2 - 1 for _ in range(planes)]
    g = [rng.random(shape) * 2 - 1 for _ in range(planes)]
    d = exponents_like(shape, rng, 2)
    d[0][:, 0] = np.nan      # element 0 along the scanned dimension is never read
    d[1][0, :] = np.nan
    pin(ins, d, [0.75, 0.5], ALL, g, f"image {shape} x {planes}")
    # one plane read along both dimensions gets both sums; a plane no scan reads gets 0
    both = [(0, True, 0), (1, False, 0)]
    d[0][:, 0] = d[0][:, 1]
    d[0][0, 0] = np.nan
    got = pin(ins, d, [0.875, 0.5], both, g, f"image {shape} x {planes}, one plane along x and y")
    assert got[1] == 0.0


def test_f64_base_gradient_of_a_signal_against_central_differences():
    rng = np.random.default_rng(2802)
    n = 40
    pin([rng.random(n) * 2 - 1], [np.concatenate([[np.nan], 0.2 + 2.0 * rng.random(n - 1)])], [0.625], PAIR_1D, [rng.random(n) * 2 - 1], "signal")


def test_f64_base_gradients_of_a_volume_against_central_differences():
    rng = np.random.default_rng(2803)
    shape = (3, 4, 8)
    ins = [rng.random(shape) * 2 - 1 for _ in range(2)]
    g = [rng.random(shape) * 2 - 1 for _ in range(2)]
    d = exponents_like(shape, rng, 3)
    d[2] += 1.5              # (a spacing along z)
    pin(ins, d, [0.75, 0.5, 0.875], VOLUME_SCANS, g, "volume")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exponents_of_infinity_and_zero(dtype):
    """d = +inf is w = 0 and contributes exactly 0 -- d is never a factor there --, d = 0 is w = 1 and contributes 0 as well: no NaN
    reaches a scalar, and the f64 loops still agree with central differences"""
    rng = np.random.default_rng(2804)
    shape = (6, 8)
    ins, g = [rng.random(shape) * 2 - 1], [rng.random(shape) * 2 - 1]
    d = exponents_like(shape, rng, 2)
    for plane in d:
        plane[rng.random(shape) < 0.15] = np.inf
        plane[rng.random(shape) < 0.15] = 0.0
    if dtype == np.float64:
        pin(ins, d, [0.75, 0.5], ALL, g, "sprinkled")
    _, got, norms = gloops.power_bases_backward(ins, d, [0.75, 0.5], ALL, g, dtype)
    assert all(np.isfinite(v) for v in got) and all(np.isfinite(n) and n > 0 for n in norms)
    # all exponents +inf: every weight is 0, every term exactly 0
    _, got, norms = gloops.power_bases_backward(ins, [np.full(shape, np.inf)] * 2, [0.75, 0.5], ALL, g, dtype)
    assert [float(v) for v in got] == [0.0, 0.0] and norms == [0.0, 0.0]


def test_f32_loops_pass_the_bar_they_define():
    """the floor of the bar is above what f32 arithmetic does to these sums"""
    rng = np.random.default_rng(2805)
    shape = (70, 132)
    ins, g = [rng.random(shape).astype(np.float32) * 2 - 1 for _ in range(2)], [rng.random(shape).astype(np.float32) * 2 - 1 for _ in range(2)]
    d = [(1.0 + 3.0 * rng.random(shape)).astype(np.float32) for _ in range(2)]
    _, want, norms = gloops.power_bases_backward(ins, d, [0.9, 0.8], ALL, g, np.float64)
    _, got, _ = gloops.power_bases_backward(ins, d, [0.9, 0.8], ALL, g, np.float32)
    for k in range(2):
        yard = gloops.figure(got[k], want[k], norms[k])
        print(f"sigma_grad_host f32 loops base {k}: figure {yard:.3e}")
        assert yard <= 1e-6


# ---- the exported surface -------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["rf_var_plan_backward_power_bases", "rf_var_plan_backward_power_bases_timed", "rf_var_plan_backward_bases_num_kernels",
               "rf_var_plan_backward_bases_workspace_bytes", "rf_smooth_plan_set_sigmas", "rf_smooth_plan_backward_sigmas",
               "rf_smooth_plan_backward_sigmas_timed", "rf_smooth_plan_backward_sigmas_num_kernels"]


def test_symbols_are_exported_declared_and_typed():
    L = capi.lib()
    header = open(rfa.capi.CSRC + "/../../include/recfilter_amd.h").read()
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes, f"{name}: no argtypes"
        assert name + "(" in header, f"{name} is not declared in recfilter_amd.h"
    assert L.rf_var_plan_backward_bases_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.rf_var_plan_backward_power_bases.argtypes) == 9 and len(L.rf_var_plan_backward_power_bases_timed.argtypes) == 12
    for name in ("backward_power_bases", "backward_power_bases_timed", "backward_bases_num_kernels", "backward_bases_workspace_bytes"):
        assert callable(getattr(rfa.VarPlan, name)), name
    assert callable(rfa.SmoothPlan.set_sigmas)
    assert capi.RF_ABI == 3 and b"abi 3" in L.rf_version()


# ---- host-only plans ------------------------------------------------------------------------------------------------------------
A, B, C, D, E, F, G = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000      # aligned, never dereferenced


def arr(values):
    return None if values is None else (ctypes.c_void_p * len(values))(*values)


def raw_bases(plan, ins, exponents, bases, grad_outs, grad_ins, grad_exponents, grad_bases, timed=False):
    L = capi.lib()
    pb = None if bases is None else (ctypes.c_float * len(bases))(*bases)
    args = [plan._h if plan is not None else None, arr(ins), arr(exponents), pb, arr(grad_outs), arr(grad_ins), arr(grad_exponents), grad_bases, None]
    if timed:
        status = L.rf_var_plan_backward_power_bases_timed(*args, (ctypes.c_float * 64)(), (ctypes.c_char_p * 64)(), 64)
    else:
        status = L.rf_var_plan_backward_power_bases(*args)
    return status, L.rf_last_error_string().decode()


@pytest.mark.parametrize("timed", [False, True])
def test_refusals_in_their_order(timed):
    """those of rf_var_plan_backward_power; null and misaligned grad_bases directly behind the null checks; RF_ERR_HIP last.  Every
    call is wrong in the way named and in everything that is checked later."""
    INV = capi.RF_ERR_INVALID_ARG
    with rfa.VarPlan((64, 64), [(0, True, 0), (1, False, 1)], planes=1, n_weights=2, device=capi.RF_DEVICE_HOST_ONLY) as plan:
        run = lambda *a: raw_bases(*a, timed=timed)      # noqa: E731
        bad = [0.5, 1.0]
        for args in ((None, None, [B, C], bad, [D], [E], None, None), (plan, None, None, bad, [D], [E], None, None),
                     (plan, None, [B, C], None, [D], [E], None, None), (plan, None, [B, C], bad, None, [E], None, None),
                     (plan, None, [B, C], bad, [D], None, None, None)):
            status, text = run(*args)
            assert status == INV and "null argument" in text, (status, text)
        # the input planes are always needed here
        for grad_exponents in (None, [None, None], [F, None]):
            status, text = run(plan, None, [B, C], bad, [D], [E], grad_exponents, None)
            assert status == INV and "in_planes" in text, (status, text)
        status, text = run(plan, [A], [B, C], bad, [D], [E], None, None)
        assert status == INV and "null grad_bases" in text, (status, text)
        for off in (1, 2, 4):
            status, text = run(plan, [A], [B, C], bad, [D], [E], None, G + off)
            assert status == INV and "8-byte aligned" in text, (status, text)
        for value in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
            status, text = run(plan, [A], [B, C], [0.5, value], [D], [D + 4], None, G)
            assert status == INV and "exponent plane 1" in text and "(0, 1)" in text, (value, status, text)
        # then the host-only plan, before alignment and overlap are looked at
        for grad_exponents in (None, [None, None], [F, None], [F + 4, F]):
            status, text = run(plan, [A], [B, C], [0.5, 0.5], [D], [D + 4], grad_exponents, G)
            assert status == capi.RF_ERR_HIP and "host-only" in text, (status, text)
        # the existing entry points answer as before
        assert plan.backward_num_kernels(False) == 6 and plan.backward_num_kernels(True) == 14


def test_timed_capacity_is_checked():
    with rfa.VarPlan((64, 64), ALL, planes=1, n_weights=2, device=capi.RF_DEVICE_HOST_ONLY) as plan:
        L = capi.lib()
        one, two = arr([A]), arr([B, C])
        status = L.rf_var_plan_backward_power_bases_timed(plan._h, one, two, (ctypes.c_float * 2)(0.5, 0.5), one, one, None, G, None,
                                                          (ctypes.c_float * 28)(), None, 28)
        assert status == capi.RF_ERR_INVALID_ARG and b"need 29" in L.rf_last_error_string()


def test_python_call_on_a_host_only_plan():
    with rfa.VarPlan((64, 64), [(0, True, 0)], planes=1, n_weights=1, device=capi.RF_DEVICE_HOST_ONLY) as plan:
        with pytest.raises(rfa.RecFilterError) as e:
            plan.backward_power_bases([], [], [0.5], [])
        assert e.value.status == capi.RF_ERR_INVALID_ARG and "grad_bases" in str(e.value)


def blocks(width, height, batch=1):
    """the workgroups of a var_grad launch: 1024 samples of a row each, at most 1024 rows on the reducing form's grid"""
    return -(-width // 1024) * min(height, 1024) * batch


def test_launch_counts_and_workspace_are_exact():
    host = capi.RF_DEVICE_HOST_ONLY
    for (H, W), planes in (((70, 132), 2), ((3, 1028), 1), ((65540, 4), 1), ((1, 4), 1)):
        with rfa.VarPlan((H, W), ALL, planes=planes, n_weights=2, device=host) as plan:
            assert plan.backward_bases_num_kernels() == 7 * 4 + 1 == plan.backward_num_kernels(True) + 1
            assert plan.backward_bases_workspace_bytes() == plan.backward_workspace_bytes(True) + 8 * 4 * blocks(W, H)
            assert plan.backward_workspace_bytes(True) == 5 * planes * H * W * 4      # (what it was)
    for n in (4, 12616):
        with rfa.VarPlan.signal(n, PAIR_1D, planes=1, n_weights=1, device=host) as plan:
            assert plan.backward_bases_num_kernels() == 15
            assert plan.backward_bases_workspace_bytes() == plan.backward_workspace_bytes(True) + 8 * 2 * blocks(n, 1)
    Dp, H, W = 6, 10, 12
    with rfa.VarPlan.volume((Dp, H, W), VOLUME_SCANS, planes=1, n_weights=3, device=host) as plan:
        assert plan.backward_bases_num_kernels() == 43
        slabs = 4 * blocks(W, H, Dp) + 2 * blocks(W * H, Dp)      # x and y stages: the slices as a batch; z: the (W * H) x D view
        assert plan.backward_bases_workspace_bytes() == plan.backward_workspace_bytes(True) + 8 * slabs


# ---- rf_smooth_plan_set_sigmas on host-only plans ---------------------------------------------------------------------------------
def host_smooth(sigma_s, sigma_r, K=3, volume=False, **kw):
    if volume:
        return rfa.SmoothPlan.volume((6, 10, 12), planes=1, iterations=K, sigma_s=sigma_s, sigma_r=sigma_r, device=capi.RF_DEVICE_HOST_ONLY, **kw)
    return rfa.SmoothPlan((64, 64), planes=1, iterations=K, sigma_s=sigma_s, sigma_r=sigma_r, device=capi.RF_DEVICE_HOST_ONLY, **kw)


def bits(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize("volume", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_set_sigmas_gives_the_bases_of_a_fresh_plan(K, volume):
    with host_smooth(60.0, 0.4, K, volume) as plan:
        before = plan.workspace_bytes, plan.num_kernels
        for sigma_s, sigma_r in ((3.0, 0.8), (17.25, 0.05), (5.5, 2.0), (60.0, 0.4)):
            plan.set_sigmas(sigma_s, sigma_r)
            with host_smooth(sigma_s, sigma_r, K, volume) as fresh:
                assert bits(plan.bases) == bits(fresh.bases), (sigma_s, sigma_r)
            assert bits(plan.bases) == bits(rfa.domain_transform_bases(sigma_s, K))
        assert (plan.workspace_bytes, plan.num_kernels) == before      # nothing is allocated, nothing else changes


def test_a_refused_set_sigmas_leaves_the_plan_unchanged():
    import torch
    INV, UNS = capi.RF_ERR_INVALID_ARG, capi.RF_ERR_UNSUPPORTED
    L = capi.lib()
    assert L.rf_smooth_plan_set_sigmas(None, 3.0, 0.8) == INV and b"null argument" in L.rf_last_error_string()
    with host_smooth(3.0, 0.8) as plan, host_smooth(3.0, 0.8, guide_planes=1, guide_dtype=torch.uint8) as byte_guided:
        for p in (plan, byte_guided):
            want = bits(p.bases)
            # create's refusals, in create's order: sigma_s, sigma_r, the scale, the bases
            for args, status, text in (((0.0, float("nan")), INV, "sigma_s"), ((float("inf"), 0.8), INV, "sigma_s"), ((-1.0, 0.8), INV, "sigma_s"),
                                       ((float("nan"), 0.8), INV, "sigma_s"), ((3.0, 0.0), INV, "sigma_r"), ((3.0, float("nan")), INV, "sigma_r"),
                                       ((3.0, -0.5), INV, "sigma_r"), ((1e300, 1e-300), UNS, "not an f32"), ((1e-3, 0.8), UNS, "a_k"),
                                       ((1e12, 0.8), UNS, "a_k")):
                with pytest.raises(rfa.RecFilterError) as e:
                    p.set_sigmas(*args)
                assert e.value.status == status and text in str(e.value), (args, e.value.status, str(e.value))
                assert bits(p.bases) == want, args
            # ... which are those create answers with
            for args, status in (((0.0, 0.8), INV), ((3.0, 0.0), INV), ((1e-3, 0.8), UNS), ((1e12, 0.8), UNS)):
                with pytest.raises(rfa.RecFilterError) as e:
                    host_smooth(*args)
                assert e.value.status == status, args


# ---- the smoothing plan's scalars: the f64 loops against central differences in sigma_s, sigma_r and spacing_z ------------------------
def smooth_loss(image, guide, sigma_s, sigma_r, K, grad_out, spacing_z):
    """L = sum(grad_out * out) of the f64 filter, nothing rounded to f32"""
    volume = spacing_z is not None
    scans = gloops.VOLUME_SCANS if volume else gloops.IMAGE_SCANS
    ds = gloops.smooth_distances(image if guide is None else guide, sigma_s, sigma_r, spacing_z, np.float64, exact=True)
    v = [np.asarray(p, dtype=np.float64) if volume else np.asarray(p, dtype=np.float64)[None] for p in image]
    for a in gloops.smooth_bases(sigma_s, K, exact=True):
        v = vloops.reference(v, [np.exp2(d * np.log2(a)) for d in ds], scans, np.float64)
    return sum(float(np.sum((np.asarray(g) if volume else np.asarray(g)[None]) * o)) for g, o in zip(grad_out, v))


@pytest.mark.parametrize("kind", ["image", "self-guided image", "volume"])
def test_f64_sigma_gradients_against_central_differences(kind):
    rng = np.random.default_rng(2806)
    volume = kind == "volume"
    shape = (2, 3, 4, 8) if volume else (2, 6, 8)
    ramps = sum(np.linspace(0, 2, n).reshape([-1 if i == ax else 1 for i in range(len(shape))]) for ax, n in enumerate(shape) if ax > 0)
    guide = 0.5 * rng.random(shape) + ramps                 # no ties: |.| is differentiable at every difference
    image = guide - 2.0 if kind == "self-guided image" else rng.random(shape) * 2 - 1
    guide = None if kind == "self-guided image" else guide
    g = rng.random(shape) * 2 - 1
    sigma_s, sigma_r, K, sz = 3.0, 0.8, 2, (2.5 if volume else None)
    got, norms = gloops.smooth_sigma_backward(image, guide, sigma_s, sigma_r, K, g, np.float64, sz, exact=True)
    L = lambda s_, r_, z_: smooth_loss(image, guide, s_, r_, K, g, z_)      # noqa: E731
    num = [(L(sigma_s + H_STEP, sigma_r, sz) - L(sigma_s - H_STEP, sigma_r, sz)) / (2 * H_STEP),
           (L(sigma_s, sigma_r + H_STEP, sz) - L(sigma_s, sigma_r - H_STEP, sz)) / (2 * H_STEP),
           (L(sigma_s, sigma_r, sz + H_STEP) - L(sigma_s, sigma_r, sz - H_STEP)) / (2 * H_STEP) if volume else 0.0]
    for j, name in enumerate(("sigma_s", "sigma_r", "spacing_z")):
        print(f"sigma_grad_host {kind} {name}: loops {got[j]:.12e}, central differences {num[j]:.12e}, sum|terms| {norms[j]:.3e}")
        assert abs(num[j] - got[j]) <= TOL * max(1.0, abs(got[j])), (kind, name, num[j], got[j])
    assert len(got) == 3 + K and all(np.isfinite(v) for v in got)
    # the f32 loops (the plan's roundings of the scale and the bases) stay under the bar they define
    want, norms = gloops.smooth_sigma_backward(image.astype(np.float32), None if guide is None else guide.astype(np.float32), sigma_s, sigma_r, K,
                                               g.astype(np.float32), np.float64, sz)
    ser, _ = gloops.smooth_sigma_backward(image.astype(np.float32), None if guide is None else guide.astype(np.float32), sigma_s, sigma_r, K,
                                          g.astype(np.float32), np.float32, sz)
    for j in range(3 + K):
        assert gloops.figure(ser[j], want[j], norms[j]) <= 1e-6, (kind, j)


# ---- rf_smooth_plan_backward_sigmas on host-only plans ------------------------------------------------------------------------------
def raw_sigmas(plan, image, guide, grad_out, grad_image, grad_guide, edges, grad_params, timed=False):
    L = capi.lib()
    args = [plan._h if plan is not None else None, arr(image), arr(guide), arr(grad_out), arr(grad_image), arr(grad_guide), edges, grad_params, None]
    if timed:
        status = L.rf_smooth_plan_backward_sigmas_timed(*args, (ctypes.c_float * 512)(), (ctypes.c_char_p * 512)(), 512)
    else:
        status = L.rf_smooth_plan_backward_sigmas(*args)
    return status, L.rf_last_error_string().decode()


@pytest.mark.parametrize("timed", [False, True])
def test_backward_sigmas_refusals_in_their_order(timed):
    """null plan / grad_out / grad_image; null, then misaligned grad_params; then those of rf_smooth_plan_backward in its order (the
    image planes always needed); RF_ERR_HIP last"""
    import torch
    INV, UNS, HIP = capi.RF_ERR_INVALID_ARG, capi.RF_ERR_UNSUPPORTED, capi.RF_ERR_HIP
    run = lambda *a: raw_sigmas(*a, timed=timed)      # noqa: E731
    with host_smooth(3.0, 0.8, guide_planes=1) as plan, host_smooth(3.0, 0.8) as self_plan, \
            host_smooth(3.0, 0.8, image_dtype=torch.uint8) as byte_plan, host_smooth(3.0, 0.8, guide_planes=1, guide_dtype=torch.uint8) as byte_guided, \
            host_smooth(3.0, 0.8, volume=True) as unflagged:
        for args in ((None, [A], [B], [C], [D], [E], 1, G), (plan, [A], [B], None, [D], [E], 1, G), (plan, [A], [B], [C], None, [E], 1, G)):
            status, text = run(*args)
            assert status == INV and "null argument" in text, (status, text)
        if not timed:      # (the timed form decides edges, the flag and the capacity before it runs)
            status, text = run(byte_plan, None, [B], [C], [D], [E], 2, None)
            assert status == INV and "null grad_params" in text, (status, text)
            status, text = run(byte_plan, None, [B], [C], [D], [E], 2, G + 4)
            assert status == INV and "8-byte aligned" in text, (status, text)
        status, text = run(byte_plan, None, [B], [C], [D], [E], 2, G)
        assert status == INV and "edges must be 0 or 1" in text, (status, text)
        status, text = run(unflagged, None, None, [C], [D], None, 1, G)
        assert status == UNS and "RF_SMOOTH_VOLUME_BACKWARD" in text, (status, text)
        status, text = run(byte_plan, None, [B], [C], [D], [E], 1, G)
        assert status == UNS and "uint8" in text, (status, text)
        status, text = run(plan, None, None, [C], [D], None, 1, G)
        assert status == INV and "guide_planes is null" in text, (status, text)
        status, text = run(self_plan, None, [B], [C], [D], [E], 1, G)
        assert status == INV and "guide_planes must be null" in text, (status, text)
        # the image planes are needed at either setting of edges
        for edges in (0, 1):
            status, text = run(plan, None, [B], [C], [D], None, edges, G)
            assert status == INV and "image_planes is null" in text, (status, text)
        status, text = run(byte_guided, [A], [B], [C], [D], None, 1, G)
        assert status == UNS and "uint8 guide" in text, (status, text)
        status, text = run(plan, [A], [B], [C], [D], None, 1, G)
        assert status == INV and "grad_guide_planes is null" in text, (status, text)
        status, text = run(plan, [A], [B], [C], [D], [E], 0, G)
        assert status == INV and "grad_guide_planes must be null" in text, (status, text)
        # then the host-only plan, before alignment and overlap are looked at; a uint8 guide is allowed without edges
        for p, args in ((plan, ([A], [B], [C], [C + 4], [A], 1, G)), (byte_guided, ([A], [B], [C], [C + 4], None, 0, G)),
                        (self_plan, ([A], None, [C], [A], None, 1, G)), (self_plan, ([A], None, [C], [A], None, 0, G))):
            status, text = run(p, *args)
            assert status == HIP and "host-only" in text, (status, text)


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_backward_sigmas_launch_counts(K):
    with host_smooth(3.0, 0.8, K) as plan, host_smooth(3.0, 0.8, K, volume=True) as unflagged, \
            rfa.SmoothPlan.volume((6, 10, 12), planes=1, iterations=K, sigma_s=3.0, sigma_r=0.8, device=capi.RF_DEVICE_HOST_ONLY, differentiable=True) as vol:
        assert plan.backward_sigmas_num_kernels(True) == plan.backward_num_kernels(True) + 2 == 34 * K - 2
        assert plan.backward_sigmas_num_kernels(False) == 34 * K - 3
        assert vol.backward_sigmas_num_kernels(True) == 51 * K - 5 and vol.backward_sigmas_num_kernels(False) == 51 * K - 6
        assert unflagged.backward_sigmas_num_kernels(True) == 0
