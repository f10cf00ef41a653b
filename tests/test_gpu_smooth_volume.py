"""GPU tests of rf_var_distances_volume and of the smoothing plan on volumes (rf_smooth_plan_create_volume; SmoothPlan.volume,
domain_transform_distances_volume, edge_aware_smooth_volume).

The distances against the f64 formula under the bound of tests/test_gpu_var_power.py (per element (C + 3) * 2^-23 of the value),
d_x and d_y bit for bit against rf_var_distances on every slice.  The f32 plan bit for bit against rf_var_distances_volume followed
by K rf_var_plan_execute_power calls on the volume plan, and against the f64 filter (tests/var_volume_loops.py on the distance
volumes the library forms) under the project's bar; byte volumes under the one-rounding rule of tests/smooth_cases.py."""
import ctypes
import functools

import numpy as np
import pytest

import guarded
import recfilter_amd as rfa
import smooth_cases as sc
import var_volume_loops as vloops
from recfilter_amd import capi

pytestmark = pytest.mark.gpu
S, R = sc.SIGMA_S, sc.SIGMA_R
SCANS = [(0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1), (2, True, 2), (2, False, 2)]
GUIDES = ["self", "u8", "f32"]      # the volume guides itself; a separate uint8 guide (3 volumes); a separate f32 guide (1 volume)
# (C, D, H, W): partial tiles along x and y with three planes; two z segments of the distance kernel and a partial z tile
SHAPES = [(3, 20, 66, 68), (1, 70, 8, 16)]
PER_ITERATION = ["var_tails_x", "var_carry", "var_pass2_x", "var_tails_y", "var_carry", "var_pass2_y", "var_tails_z", "var_carry", "var_pass2_z"]


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def guide_of(shape, kind):
    if kind == "u8":
        return sc.byte_image((3,) + shape[1:], "guide")
    if kind == "f32":
        return sc.float_image((1,) + shape[1:], "guide")
    return None


# ---- the distances --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", [1.0, 2.5])
@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("shape", [(1, 20, 66, 68), (3, 20, 66, 68), (16, 33, 5, 8), (1, 1, 40, 64)], ids=str)
def test_distances_against_the_f64_formula(shape, kind, spacing):
    import torch
    C = shape[0]
    g = sc.byte_image(shape, "guide") if kind == "u8" else sc.float_image(shape, "guide")
    got = rfa.domain_transform_distances_volume(dev(g), S, R, spacing_z=spacing)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in got]
    want = vloops.distances(g.astype(np.float64) / (255.0 if kind == "u8" else 1.0), S / R, spacing, np.float64)
    bound = (C + 3) * 2.0 ** -23
    for axis, a, w in zip("xyz", got, want):
        assert a.dtype == np.float32 and not np.isnan(a).any(), f"d_{axis}"
        rel = float(np.max(np.abs(a.astype(np.float64) - w) / w))
        print(f"distances {shape} {kind} spacing {spacing}: d_{axis} max relative error {rel:.3e}, bound {bound:.3e}")
        assert rel <= bound, f"d_{axis} is {rel:.3e} off, bound {bound:.3e}"
    np.testing.assert_array_equal(got[0][:, :, 0], np.float32(1))
    np.testing.assert_array_equal(got[1][:, 0, :], np.float32(1))
    np.testing.assert_array_equal(got[2][0], np.float32(spacing))
    # d_x and d_y: what the image entry point gives on every slice
    for z in range(shape[1]):
        dx, dy = rfa.domain_transform_distances(dev(np.ascontiguousarray(g[:, z])), S, R)
        np.testing.assert_array_equal(got[0][z].view(np.uint32), dx.cpu().numpy().view(np.uint32), err_msg=f"d_x of slice {z}")
        np.testing.assert_array_equal(got[1][z].view(np.uint32), dy.cpu().numpy().view(np.uint32), err_msg=f"d_y of slice {z}")


def test_distances_of_a_single_volume_and_guards():
    """a (D, H, W) guide; the three outputs stay inside their volumes and the guide is unchanged"""
    import torch
    shape = (20, 66, 68)
    g = sc.float_image((1,) + shape, "guide")
    d_g, c_g = guarded.guarded_planes(shape, np.float32, 1, fill=guarded.IN_FILL)
    d_out, c_out = guarded.guarded_planes(shape, np.float32, 3, fill=guarded.OUT_FILL)
    c_g.load([torch.from_numpy(np.array(g[0]))])
    c_g.snapshot()
    arr = (ctypes.c_void_p * 1)(d_g[0].data_ptr())
    D, H, W = shape
    capi.check(capi.lib().rf_var_distances_volume(arr, 1, 0, W, H, D, S / R, 2.5, d_out[0].data_ptr(), d_out[1].data_ptr(), d_out[2].data_ptr(), -1,
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    c_out.check_guards("distances")
    c_g.check_unchanged("guide")
    want = rfa.domain_transform_distances_volume(dev(g[0]), S, R, spacing_z=2.5)
    for a, b in zip(d_out, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_distance_refusals_on_a_device():
    import torch
    D, H, W = 4, 8, 16
    g = torch.zeros((D, H, W), device="cuda")
    out = torch.zeros((3, D, H, W), device="cuda")
    lib = capi.lib()

    def status(guide, dx, dy, dz, u8=0, spacing=1.0):
        arr = (ctypes.c_void_p * 1)(guide)
        return lib.rf_var_distances_volume(arr, 1, u8, W, H, D, 1.0, spacing, dx, dy, dz, -1, None)
    p = [out[k].data_ptr() for k in range(3)]
    assert status(g.data_ptr(), p[0], p[1], p[1]) == capi.RF_ERR_INVALID_ARG                 # dz is dy
    assert status(g.data_ptr(), p[0], p[1], g.data_ptr()) == capi.RF_ERR_INVALID_ARG         # dz is the guide
    assert status(g.data_ptr(), p[0], p[1], p[2] + 4) == capi.RF_ERR_INVALID_ARG             # alignment
    assert status(g.data_ptr() + 2, p[0], p[1], p[2], u8=1) == capi.RF_ERR_INVALID_ARG
    assert status(g.data_ptr(), p[0], p[1], p[2], spacing=0.0) == capi.RF_ERR_INVALID_ARG
    assert status(g.data_ptr(), p[0], p[1], p[2]) == capi.RF_OK
    torch.cuda.synchronize()


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def make_plan(shape, image, guide, K, spacing):
    import torch
    to_torch = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32}
    return rfa.SmoothPlan.volume(shape[1:], planes=shape[0], guide_planes=0 if guide is None else guide.shape[0], image_dtype=to_torch[image.dtype],
                                 guide_dtype=None if guide is None else to_torch[guide.dtype], iterations=K, sigma_s=S, sigma_r=R, spacing_z=spacing)


def run_plan(shape, image, guide, K, spacing, inplace=False):
    """(result on the host, the plan's bases)"""
    import torch
    with make_plan(shape, image, guide, K, spacing) as plan:
        src = dev(image)
        out = plan.execute(src, None if guide is None else dev(guide), src if inplace else None)
        torch.cuda.synchronize()
        return out.cpu().numpy(), [np.float32(b) for b in plan.bases]


def library_distances(image, guide, spacing):
    import torch
    ds = rfa.domain_transform_distances_volume(dev(image if guide is None else guide), S, R, spacing_z=spacing)
    torch.cuda.synchronize()
    return [d.cpu().numpy() for d in ds]


@functools.lru_cache(maxsize=None)
def library_bases(K):
    with rfa.SmoothPlan.volume((8, 40, 64), iterations=K, sigma_s=S, sigma_r=R, device=capi.RF_DEVICE_HOST_ONLY) as plan:
        return [np.float32(b) for b in plan.bases]


def filter_loops(image, ds, bases, dtype):
    volumes = [np.asarray(p, dtype=dtype) for p in image]
    for a in bases:
        volumes = vloops.reference(volumes, vloops.power_weights(ds, [a, a, a], dtype), SCANS, dtype)
    return np.stack(volumes)


@functools.lru_cache(maxsize=None)
def expected(shape, image_kind, guide_kind, K, spacing):
    """(volume, guide, f64 truth, the f32 serial loops' max abs error) on the distance volumes and the bases the library reports"""
    image = sc.byte_image(shape) if image_kind == "u8" else sc.float_image(shape)
    guide = guide_of(shape, guide_kind)
    ds = library_distances(image, guide, spacing)
    want = filter_loops(image, ds, library_bases(K), np.float64)
    serial = filter_loops(image, ds, library_bases(K), np.float32)
    want.setflags(write=False)
    return image, guide, want, float(np.max(np.abs(serial.astype(np.float64) - want)))


def test_the_bases_are_the_image_plan_s():
    with rfa.SmoothPlan((40, 64), iterations=3, sigma_s=S, sigma_r=R, device=capi.RF_DEVICE_HOST_ONLY) as plan:
        assert [np.float32(b) for b in plan.bases] == library_bases(3)


@pytest.mark.parametrize("spacing", [1.0, 2.5])
@pytest.mark.parametrize("guide_kind", GUIDES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_f32_equals_the_calls_written_out(shape, guide_kind, spacing):
    import torch
    K = 3
    C = shape[0]
    image, guide = sc.float_image(shape), guide_of(shape, guide_kind)
    got, bases = run_plan(shape, image, guide, K, spacing)
    ds = list(rfa.domain_transform_distances_volume(dev(image if guide is None else guide), S, R, spacing_z=spacing))
    src = [t.contiguous() for t in dev(image)]
    with rfa.VarPlan.volume(shape[1:], SCANS, planes=C, n_weights=3) as plan:
        for a in bases:
            src = plan.execute_power(src, ds, [a, a, a])
        torch.cuda.synchronize()
    guarded.assert_bits_equal([torch.from_numpy(got[c]) for c in range(C)], [t.cpu() for t in src],
                              f"SmoothPlan.volume {shape} guide {guide_kind} against the distances + {K} x execute_power")
    assert bases == library_bases(K)


@pytest.mark.parametrize("guide_kind", GUIDES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_f32_against_the_f64_filter(shape, guide_kind):
    image, guide, want, abs_err32 = expected(shape, "f32", guide_kind, 3, 2.5)
    got, _ = run_plan(shape, image, guide, 3, 2.5)
    peak = float(np.max(np.abs(image)))
    assert sc.f32_bar_excess(got, want, abs_err32, peak, f"f32 volume {shape} guide {guide_kind}") <= 0
    assert float(np.max(np.abs(got - image))) > 0.05, "the filter left the volume"


@pytest.mark.parametrize("guide_kind", GUIDES)
@pytest.mark.parametrize("shape,K", [(SHAPES[0], 3), (SHAPES[1], 1), (SHAPES[1], 3)], ids=str)
def test_bytes_under_the_one_rounding_rule(shape, K, guide_kind):
    image, guide, want, abs_err32 = expected(shape, "u8", guide_kind, K, 1.0)
    got, bases = run_plan(shape, image, guide, K, 1.0)
    assert bases == library_bases(K)
    assert sc.byte_rule_excess(got, want, abs_err32, f"byte volume {shape} K = {K} guide {guide_kind}") <= 0
    assert (got != image).mean() > 0.5, "the filter left the volume"


@pytest.mark.parametrize("image_kind", ["u8", "f32"])
def test_in_place_equals_out_of_place_and_no_state_is_kept(image_kind):
    import torch
    shape = SHAPES[0]
    image = sc.byte_image(shape) if image_kind == "u8" else sc.float_image(shape)
    a, _ = run_plan(shape, image, None, 3, 2.5)
    b, _ = run_plan(shape, image, None, 3, 2.5, inplace=True)
    np.testing.assert_array_equal(a, b)
    with make_plan(shape, image, None, 3, 2.5) as plan:
        first = plan.execute(dev(image)).cpu().numpy()
        plan.execute(dev(np.full(shape, 255 if image_kind == "u8" else np.nan, dtype=image.dtype)))
        third = plan.execute(dev(image)).cpu().numpy()
        torch.cuda.synchronize()
    np.testing.assert_array_equal(first, third)
    np.testing.assert_array_equal(first, a)


@pytest.mark.parametrize("image_kind", ["u8", "f32"])
def test_guarded_volumes(image_kind):
    import torch
    shape = SHAPES[0]
    dtype = np.uint8 if image_kind == "u8" else np.float32
    image = sc.byte_image(shape) if image_kind == "u8" else sc.float_image(shape)
    d_in, c_in = guarded.guarded_planes(shape[1:], dtype, shape[0], fill=guarded.IN_FILL)
    d_out, c_out = guarded.guarded_planes(shape[1:], dtype, shape[0], fill=guarded.OUT_FILL)
    c_in.load([torch.from_numpy(np.array(p)) for p in image])
    c_in.snapshot()
    with make_plan(shape, image, None, 3, 1.0) as plan:
        plan.execute(d_in, None, d_out)
        torch.cuda.synchronize()
    c_out.check_guards("output")
    c_in.check_unchanged("input")
    want, _ = run_plan(shape, image, None, 3, 1.0)
    np.testing.assert_array_equal(np.stack([t.cpu().numpy() for t in d_out]), want)


@pytest.mark.parametrize("image_kind", ["u8", "f32"])
def test_timed_names_the_launch_list(image_kind):
    shape, K = SHAPES[1], 3
    image = sc.byte_image(shape) if image_kind == "u8" else sc.float_image(shape)
    with make_plan(shape, image, None, K, 1.0) as plan:
        out, report = plan.execute_timed(dev(image))
        assert [n for n, _ in report] == ["var_distances_volume"] + PER_ITERATION * K
        assert plan.num_kernels == 1 + 9 * K
        assert all(ms > 0 for _, ms in report)
        np.testing.assert_array_equal(out.cpu().numpy(), plan.execute(dev(image)).cpu().numpy())


@pytest.mark.parametrize("image_kind", ["u8", "f32"])
@pytest.mark.parametrize("guide_kind", ["self", "u8"])
def test_edge_aware_smooth_volume(image_kind, guide_kind):
    import torch
    shape, K = SHAPES[0], 3
    image = sc.byte_image(shape) if image_kind == "u8" else sc.float_image(shape)
    guide = guide_of(shape, guide_kind)
    want, _ = run_plan(shape, image, guide, K, 2.5)
    got = rfa.edge_aware_smooth_volume(dev(image), None if guide is None else dev(guide), sigma_s=S, sigma_r=R, iterations=K, spacing_z=2.5)
    torch.cuda.synchronize()
    assert got.dtype == (torch.uint8 if image_kind == "u8" else torch.float32)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    one = rfa.edge_aware_smooth_volume(dev(image)[0], dev(image), sigma_s=S, sigma_r=R, iterations=K)      # (D, H, W)
    assert tuple(one.shape) == shape[1:]


def test_backward_is_refused():
    import torch
    shape = SHAPES[1]
    image = dev(sc.float_image(shape))
    with make_plan(shape, sc.float_image(shape), None, 3, 1.0) as plan:
        for edges in (False, True):
            with pytest.raises(rfa.RecFilterError) as e:
                plan.backward(image, None, torch.ones_like(image), edges=edges)
            assert e.value.status == capi.RF_ERR_UNSUPPORTED
        assert plan.backward_num_kernels(False) == 0 and plan.backward_workspace_bytes(True) == 0
