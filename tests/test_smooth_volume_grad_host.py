"""CPU tests of the differentiable smoothing plan on volumes (RF_SMOOTH_VOLUME_BACKWARD, rf_var_distances_volume_backward): the loops
of tests/smooth_volume_grad_loops.py -- the yardstick of tests/test_gpu_smooth_volume_grad.py -- pinned by central differences and by
torch's autograd in f64 and held to the project's bar in f32, and what the library decides without a device: launch counts, the
exact name lists, the workspace formula, the flag's rules at create and every refusal in its documented order on host-only plans
and through addresses that are never dereferenced.  No kernel is launched."""
import ctypes

import numpy as np
import pytest

import recfilter_amd as rfa
import smooth_volume_grad_cases as cases
import smooth_volume_grad_loops as vsloops
import var_volume_loops as vloops
from recfilter_amd import capi

HOST = capi.RF_DEVICE_HOST_ONLY
INV, UNS, HIP = capi.RF_ERR_INVALID_ARG, capi.RF_ERR_UNSUPPORTED, capi.RF_ERR_HIP


# ---- the loops ------------------------------------------------------------------------------------------------------------------
def small_case():
    """a (2, 5, 6, 8) volume, a guide without ties, K = 2"""
    shape = (2, 5, 6, 8)
    rng = np.random.default_rng(2027)
    image, g_out = rng.random(shape) * 2 - 1, rng.random(shape) * 2 - 1
    guide = 0.5 * rng.random(shape) + np.linspace(0, 1, 8) + np.linspace(0, 1, 6)[:, None] + np.linspace(0, 1, 5)[:, None, None]
    bases = [np.float32(0.8), np.float32(0.9)]
    return image, guide, g_out, bases, 1.5, 2.5


def test_distance_adjoint_against_central_differences():
    """<gdx, d_x> + <gdy, d_y> + <gdz, d_z> as a function of the guide, along a random direction, in f64"""
    image, guide, _, _, scale, spacing = small_case()
    rng = np.random.default_rng(3)
    gd = [rng.random(guide.shape[1:]) * 2 - 1 for _ in range(3)]
    direction, h = rng.random(guide.shape) * 2 - 1, 1e-7

    def loss(g):
        return sum(float(np.sum(a * d)) for a, d in zip(gd, vloops.distances(g, scale, spacing, np.float64)))
    got = vsloops.distances_backward(guide, scale, gd[0], gd[1], gd[2], np.float64)
    fd = (loss(guide + h * direction) - loss(guide - h * direction)) / (2 * h)
    assert abs(fd - float(np.sum(got * direction))) < 1e-6
    # the faces: gdx[:, :, 0], gdy[:, 0, :] and gdz[0] reach nothing
    poisoned = [a.copy() for a in gd]
    poisoned[0][:, :, 0], poisoned[1][:, 0, :], poisoned[2][0] = np.nan, np.nan, np.nan
    np.testing.assert_array_equal(vsloops.distances_backward(guide, scale, *poisoned, np.float64), got)


@pytest.mark.parametrize("self_guided", [False, True])
def test_whole_backward_against_central_differences(self_guided):
    """L = sum(g_out * filter(image, guide)): directional derivatives in the image, in the guide and in each distance volume"""
    image, guide, g_out, bases, scale, spacing = small_case()
    rng = np.random.default_rng(4)
    d_im, d_gd, h = rng.random(image.shape) * 2 - 1, rng.random(guide.shape) * 2 - 1, 1e-6

    def run(im, gd, ds=None):
        ds = vloops.distances(im if gd is None else gd, scale, spacing, np.float64) if ds is None else ds
        return float(np.sum(g_out * np.stack(vsloops.smooth_forward(im, ds, bases, np.float64)[-1])))
    gd_arg = None if self_guided else guide
    grad_im, grad_gd, grad_ds = vsloops.smooth_backward(image, gd_arg, bases, scale, spacing, g_out, np.float64, True)
    fd = (run(image + h * d_im, gd_arg) - run(image - h * d_im, gd_arg)) / (2 * h)
    assert abs(fd - float(np.sum(grad_im * d_im))) < 1e-6, "image"
    if not self_guided:
        fd = (run(image, guide + h * d_gd) - run(image, guide - h * d_gd)) / (2 * h)
        assert abs(fd - float(np.sum(grad_gd * d_gd))) < 1e-6, "guide"
        held, none, _ = vsloops.smooth_backward(image, guide, bases, scale, spacing, g_out, np.float64, False)
        assert none is None
        np.testing.assert_array_equal(held, grad_im)      # the image gradient does not depend on edges with a separate guide
    # each distance volume, element 0 along its axis left out (it is never read, and its gradient is exactly 0)
    ds = vloops.distances(image if self_guided else guide, scale, spacing, np.float64)
    for k, axis in enumerate((2, 1, 0)):
        direction = rng.random(ds[k].shape) * 2 - 1
        shifted = lambda t: [d + t * direction if q == k else d for q, d in enumerate(ds)]      # noqa: E731
        fd = (run(image, gd_arg, shifted(h)) - run(image, gd_arg, shifted(-h))) / (2 * h)
        assert np.all(np.take(grad_ds[k], 0, axis=axis) == 0)
        assert abs(fd - float(np.sum(np.delete(grad_ds[k] * direction, 0, axis=axis)))) < 1e-6, f"distance volume {k}"


@pytest.mark.parametrize("self_guided", [False, True])
def test_loops_against_torch_autograd(self_guided):
    import torch
    image, guide, g_out, bases, scale, spacing = small_case()
    im = torch.from_numpy(image).requires_grad_(True)
    gd = None if self_guided else torch.from_numpy(guide).requires_grad_(True)
    out = vsloops.torch_filter(im, gd, bases, scale, spacing, torch.float64)
    ds = vloops.distances(image if self_guided else guide, scale, spacing, np.float64)
    np.testing.assert_allclose(out.detach().numpy(), np.stack(vsloops.smooth_forward(image, ds, bases, np.float64)[-1]), rtol=0, atol=1e-13)
    out.backward(torch.from_numpy(g_out))
    grad_im, grad_gd, _ = vsloops.smooth_backward(image, None if self_guided else guide, bases, scale, spacing, g_out, np.float64, True)
    np.testing.assert_allclose(im.grad.numpy(), grad_im, rtol=0, atol=1e-12)
    if not self_guided:
        np.testing.assert_allclose(gd.grad.numpy(), grad_gd, rtol=0, atol=1e-12)


def test_a_constant_guide_gets_exactly_zero():
    """sgn(0) = 0, in the loops and in torch"""
    import torch
    image, _, g_out, bases, scale, spacing = small_case()
    guide = np.full(image.shape, 0.375)
    _, grad_gd, _ = vsloops.smooth_backward(image, guide, bases, scale, spacing, g_out, np.float64, True)
    np.testing.assert_array_equal(grad_gd, np.zeros_like(guide))
    gd = torch.from_numpy(guide).requires_grad_(True)
    vsloops.torch_filter(torch.from_numpy(image), gd, bases, scale, spacing, torch.float64).backward(torch.from_numpy(g_out))
    np.testing.assert_array_equal(gd.grad.numpy(), np.zeros_like(guide))
    rng = np.random.default_rng(5)
    gds = [rng.random(image.shape[1:]) for _ in range(3)]
    np.testing.assert_array_equal(vsloops.distances_backward(guide, scale, *gds, np.float32), np.zeros(image.shape, dtype=np.float32))


@pytest.mark.parametrize("order", ["plan", "forward"])
@pytest.mark.parametrize("self_guided", [False, True])
def test_f32_loops_pass_the_bar_in_either_order(order, self_guided):
    """the f32 loops with the distance gradients summed in the other order stay under the bar the GPU is held to"""
    shape, K = cases.SHAPES[1], 3
    kind = "self" if self_guided else "f32"
    want_im, want_gd, err_im, err_gd = cases.expected(shape, K, kind, True)
    got = vsloops.smooth_backward(cases.image(shape), None if self_guided else cases.guide(shape), cases.bases(K), cases.SCALE, cases.SPACING_Z,
                                  cases.grad_out(shape), np.float32, True, order=order)
    cases.assert_under_bar([got[0]], [want_im], err_im, f"f32 loops, order {order}, image")
    if not self_guided:
        cases.assert_under_bar([got[1]], [want_gd], err_gd, f"f32 loops, order {order}, guide")


def test_the_case_names_count_as_documented():
    for K in (1, 2, 3, 8):
        assert len(cases.expected_names(K, False)) == 1 + 18 * K
        assert len(cases.expected_names(K, True)) == 51 * K - 7


# ---- host-only plans ------------------------------------------------------------------------------------------------------------
def host_volume(shape=(8, 40, 64), planes=1, guide_planes=0, K=2, image_dtype=None, guide_dtype=None, differentiable=True):
    return rfa.SmoothPlan.volume(shape, planes=planes, guide_planes=guide_planes, image_dtype=image_dtype, guide_dtype=guide_dtype, iterations=K,
                                 sigma_s=cases.SIGMA_S, sigma_r=cases.SIGMA_R, spacing_z=cases.SPACING_Z, device=HOST, differentiable=differentiable)


def arr(values):
    return None if values is None else (ctypes.c_void_p * len(values))(*values)


def message():
    return capi.lib().rf_last_error_string().decode()


def timed_names(plan, edges=None):
    """the launch names of a host-only plan: the timed entry points fill names_out before they refuse to run"""
    n = plan.num_kernels if edges is None else plan.backward_num_kernels(edges)
    ms, names = (ctypes.c_float * n)(), (ctypes.c_char_p * n)()
    nulls = lambda k: (ctypes.c_void_p * max(k, 1))()      # noqa: E731
    guide = nulls(plan.guide_planes) if plan.guide_planes else None
    if edges is None:
        status = capi.lib().rf_smooth_plan_execute_timed(plan._h, nulls(plan.planes), guide, nulls(plan.planes), None, ms, names, n)
    else:
        status = capi.lib().rf_smooth_plan_backward_timed(plan._h, nulls(plan.planes), guide, nulls(plan.planes), nulls(plan.planes),
                                                          guide if edges else None, int(edges), None, ms, names, n)
    assert status == HIP, message()
    return [v.decode() for v in names]


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("planes,guide_planes", [(1, 0), (3, 0), (3, 1)])
def test_launch_counts_names_and_workspace(K, planes, guide_planes):
    shape = (20, 66, 68)
    samples = int(np.prod(shape))
    with host_volume(shape, planes, guide_planes, K) as plan, host_volume(shape, planes, guide_planes, K, differentiable=False) as plain:
        assert plan.backward_num_kernels(False) == 1 + 18 * K
        assert plan.backward_num_kernels(True) == 51 * K - 7
        assert timed_names(plan, False) == cases.expected_names(K, False)
        assert timed_names(plan, True) == cases.expected_names(K, True)
        assert plan.backward_workspace_bytes(False) == 0
        assert plan.backward_workspace_bytes(True) == (3 + (K - 1 + 7) * planes) * samples * 4
        # the forward is the unflagged plan's
        assert plan.num_kernels == plain.num_kernels == 1 + 9 * K
        assert plan.workspace_bytes == plain.workspace_bytes
        assert timed_names(plan) == timed_names(plain)
        assert plan.bases == plain.bases
        # and the unflagged plan is what it was
        assert plain.backward_num_kernels(False) == 0 and plain.backward_num_kernels(True) == 0 and plain.backward_workspace_bytes(True) == 0


def test_timed_capacity_is_checked():
    with host_volume(K=2) as plan:
        L = capi.lib()
        one = arr([0x10000])
        for edges, need in ((0, 37), (1, 95)):
            status = L.rf_smooth_plan_backward_timed(plan._h, one, None, one, one, None, edges, None, (ctypes.c_float * 5)(), None, 5)
            assert status == INV and f"need {need}".encode() in L.rf_last_error_string()


def raw_create(flags, image_u8=0, guide_u8=0, n_guide=0):
    d = capi.SmoothVolumeDesc()
    d.abi, d.image_u8, d.width, d.height, d.depth = capi.RF_ABI, image_u8, 64, 40, 8
    d.n_planes, d.n_guide, d.guide_u8, d.iterations = 1, n_guide, guide_u8, 2
    d.sigma_s, d.sigma_r, d.spacing_z = 40.0, 0.5, 1.0
    d.device, d.flags = HOST, flags
    h = ctypes.c_void_p()
    status = capi.lib().rf_smooth_plan_create_volume(ctypes.byref(d), ctypes.byref(h))
    text = message()
    if status == capi.RF_OK:
        capi.lib().rf_smooth_plan_destroy(h)
    else:
        assert not h.value, "a refused description must not leave a plan behind"
    return status, text


def test_the_flag_at_create():
    assert capi.RF_SMOOTH_VOLUME_BACKWARD == 1
    assert raw_create(0)[0] == capi.RF_OK
    assert raw_create(1)[0] == capi.RF_OK
    for flags in (2, 3, 0x80000000, 0x80000001):
        status, text = raw_create(flags)
        assert status == INV and "flags" in text, (flags, status, text)
    status, text = raw_create(1, image_u8=1)
    assert status == UNS and "RF_SMOOTH_VOLUME_BACKWARD" in text, (status, text)
    assert raw_create(0, image_u8=1)[0] == capi.RF_OK
    # a byte guide is accepted at create (and refused at an edges = 1 call)
    assert raw_create(1, guide_u8=1, n_guide=3)[0] == capi.RF_OK
    import torch
    with pytest.raises(rfa.RecFilterError) as e:
        host_volume(image_dtype=torch.uint8)
    assert e.value.status == UNS


A, B, C, D, E, F = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000      # 16-byte aligned, never dereferenced; 8 x 40 x 64 f32: 0x14000 bytes


def raw_smooth(plan, image, guide, grad_out, grad_image, grad_guide, edges, timed=False):
    L = capi.lib()
    args = [plan._h if plan is not None else None, arr(image), arr(guide), arr(grad_out), arr(grad_image), arr(grad_guide), edges, None]
    if timed:
        status = L.rf_smooth_plan_backward_timed(*args, (ctypes.c_float * 512)(), (ctypes.c_char_p * 512)(), 512)
    else:
        status = L.rf_smooth_plan_backward(*args)
    return status, message()


@pytest.mark.parametrize("timed", [False, True])
def test_backward_refusals_in_their_order(timed):
    """those documented for rf_smooth_plan_backward, on flagged volume plans; the volume refusal only without the flag, at its place"""
    import torch
    run = lambda *a: raw_smooth(*a, timed=timed)      # noqa: E731
    with host_volume(guide_planes=1) as plan, host_volume() as self_plan, host_volume(guide_planes=1, guide_dtype=torch.uint8) as byte_guide_plan, \
            host_volume(differentiable=False) as plain, host_volume(image_dtype=torch.uint8, differentiable=False) as plain_bytes:
        for args in ((None, [A], [B], [C], [D], [E], 1), (plan, [A], [B], None, [D], [E], 1), (plan, [A], [B], [C], None, [E], 1)):
            status, text = run(*args)
            assert status == INV and "null argument" in text, (status, text)
        for edges in (-1, 2):
            for p in (plan, plain):
                status, text = run(p, None, [B], [C], [D], [E], edges)
                assert status == INV and "edges must be 0 or 1" in text, (status, text)
        # a plan without the flag, whatever else is wrong (a byte-volume plan cannot carry the flag)
        for p in (plain, plain_bytes):
            for edges in (0, 1):
                status, text = run(p, None, [B], [C], [D], [E], edges)
                assert status == UNS and "RF_SMOOTH_VOLUME_BACKWARD" in text, (status, text)
        status, text = run(plan, None, None, [C], [D], None, 1)
        assert status == INV and "guide_planes is null" in text, (status, text)
        status, text = run(self_plan, None, [B], [C], [D], [E], 1)
        assert status == INV and "guide_planes must be null" in text, (status, text)
        # the volumes: needed through the distances, and where the volume guides itself
        status, text = run(plan, None, [B], [C], [D], None, 1)
        assert status == INV and "image_planes is null" in text, (status, text)
        status, text = run(self_plan, None, None, [C], [D], [E], 0)
        assert status == INV and "image_planes is null" in text, (status, text)
        # a byte guide: refused only through the distances
        status, text = run(byte_guide_plan, [A], [B], [C], [D], None, 1)
        assert status == UNS and "uint8 guide" in text, (status, text)
        status, text = run(byte_guide_plan, None, [B], [C], [D], None, 0)
        assert status == HIP and "host-only" in text, (status, text)
        # the guide's gradient volumes: required with a separate guide through the distances, refused everywhere else
        status, text = run(plan, [A], [B], [C], [D], None, 1)
        assert status == INV and "grad_guide_planes is null" in text, (status, text)
        status, text = run(plan, [A], [B], [C], [D], [E], 0)
        assert status == INV and "grad_guide_planes must be null" in text, (status, text)
        status, text = run(self_plan, [A], None, [C], [D], [E], 1)
        assert status == INV and "grad_guide_planes must be null" in text, (status, text)
        # then the host-only plan, before alignment and overlap are looked at
        for p, args in ((plan, ([A], [B], [C], [C + 4], [A], 1)), (plan, (None, [B], [C], [C + 4], None, 0)),
                        (self_plan, ([A], None, [C], [A], None, 1)), (self_plan, ([A], None, [C], [A], None, 0))):
            status, text = run(p, *args)
            assert status == HIP and "host-only" in text, (status, text)


def test_python_backward_on_host_only_plans():
    with host_volume(guide_planes=1) as plan:
        with pytest.raises(rfa.RecFilterError) as e:
            plan.backward([], [], [], edges=False)
        assert e.value.status == HIP
        with pytest.raises(rfa.RecFilterError) as e:
            plan.backward_timed([], [], [], None, [], edges=True)
        assert e.value.status == HIP


# ---- rf_var_distances_volume_backward: what is decided before any HIP call ----------------------------------------------------------
def raw_distances_backward(guide, n_guide, W, H, Dp, scale, gdx, gdy, gdz, grads, accumulate=0):
    status = capi.lib().rf_var_distances_volume_backward(arr(guide), n_guide, W, H, Dp, scale, gdx, gdy, gdz, arr(grads), accumulate, -1, None)
    return status, message()


def test_distances_backward_refusals_are_decided_without_a_device():
    """every refusal, in order: each call is wrong in the way named and in everything that is checked later"""
    run = raw_distances_backward
    G = 0x700000
    for n in (0, capi.RF_MAX_PLANES + 1):
        assert run(None, n, 0, 0, 0, -1.0, None, None, None, None)[0] == INV and "n_guide" in message()
    for W, H, Dp in ((0, 40, 8), (64, 0, 8), (64, 40, 0), (64, 40, -1)):
        assert run(None, 1, W, H, Dp, -1.0, None, None, None, None)[0] == INV and "positive" in message()
    for args in ((None, B, C, D, [E]), ([A], None, C, D, [E]), ([A], B, None, D, [E]), ([A], B, C, None, [E]), ([A], B, C, D, None)):
        assert run(args[0], 1, 62, 40, 8, -1.0, args[1], args[2], args[3], args[4])[0] == INV and "null argument" in message()
    for guide, grads in (([A, None], [E, F]), ([A, G], [E, None])):
        assert run(guide, 2, 62, 40, 8, -1.0, B, C, D, grads)[0] == INV and "guide volume 1: null pointer" in message()
    for scale in (-1.0, float("nan"), float("inf")):
        assert run([A], 1, 62, 40, 8, scale, B, C, D, [E], 2)[0] == INV and "scale" in message()
    # the volume domain of the forward, n_planes = 1
    assert run([A], 1, 62, 40, 8, 1.0, B + 4, C, D, [E], 2)[0] == UNS and "multiple of 4" in message()
    assert run([A], 1, 64, (1 << 21) + 1, 8, 1.0, B + 4, C, D, [E], 2)[0] == UNS and "above" in message()
    assert run([A], 1, 1 << 15, (1 << 15) + 1, 1, 1.0, B + 4, C, D, [E], 2)[0] == UNS and "width * height" in message()
    assert run([A], 1, 64, 40, 65536, 1.0, B + 4, C, D, [E], 2)[0] == UNS and "depth" in message()
    for accumulate in (2, -1):
        assert run([A], 1, 64, 40, 8, 1.0, B + 4, C, D, [E], accumulate)[0] == INV and "accumulate" in message()
    for gd in ((B + 4, C, D), (B, C + 8, D), (B, C, D + 4)):
        assert run([A + 4], 1, 64, 40, 8, 1.0, *gd, [E])[0] == INV and "grad_dx, grad_dy and grad_dz" in message()
    for guide, grads in (([A + 4], [B]), ([A], [B + 8])):
        assert run(guide, 1, 64, 40, 8, 1.0, B, C, D, grads)[0] == INV and "guide volume 0" in message() and "16-byte" in message()
    # overlaps: 8 x 40 x 64 f32 volumes are 0x14000 bytes
    assert run([A], 1, 64, 40, 8, 1.0, B, C, D, [B + 0x13ff0])[0] == INV and "gradient of guide volume 0 overlaps grad_dx, grad_dy or grad_dz" in message()
    assert run([A], 1, 64, 40, 8, 1.0, B, C, D, [C])[0] == INV and "grad_dx, grad_dy or grad_dz" in message()
    assert run([A], 1, 64, 40, 8, 1.0, B, C, D, [D])[0] == INV and "grad_dx, grad_dy or grad_dz" in message()
    assert run([A, G], 2, 64, 40, 8, 1.0, B, C, D, [E, G + 0x1000])[0] == INV and "gradient of guide volume 1 overlaps guide volume 1" in message()
    assert run([A, G], 2, 64, 40, 8, 1.0, B, C, D, [E, A])[0] == INV and "gradient of guide volume 1 overlaps guide volume 0" in message()
    assert run([A, G], 2, 64, 40, 8, 1.0, B, C, D, [E, E + 0x100])[0] == INV and "gradient of guide volume 0 overlaps gradient of guide volume 1" in message()


# ---- the exported surface -------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_typed():
    L = capi.lib()
    header = open(rfa.capi.CSRC + "/../../include/recfilter_amd.h").read()
    name = "rf_var_distances_volume_backward"
    assert name in capi.EXPORTED_SYMBOLS
    assert len(getattr(L, name).argtypes) == 13
    assert name + "(" in header and "#define RF_SMOOTH_VOLUME_BACKWARD 1u" in header
    assert capi.RF_ABI == 3 and b"abi 3" in L.rf_version()
    assert "domain_transform_distances_volume_backward" in rfa.__all__
