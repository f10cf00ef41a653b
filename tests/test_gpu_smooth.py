"""GPU tests of the smoothing plan (rf_smooth_plan_*, recfilter_amd.SmoothPlan, edge_aware_smooth(form="plan"),
RecFilterSmooth): f32 images bit for bit against rf_var_distances followed by K rf_var_plan_execute_power calls; byte images
under the one-rounding rule of tests/smooth_cases.py against the f64 loops on the distance planes the library forms from the
same guide; exact cases, in place, state, guarded planes, the launch names, the refusals at execute, the whole filter on a noisy
step, and the C++ front-end."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import guarded
import recfilter_amd as rfa
import smooth_cases as sc
import test_gpu_var_power as power            # smooth_case and assert_step_kept_noise_gone (the module, not its tests)
from recfilter_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, R = sc.SIGMA_S, sc.SIGMA_R
EXACT = (1, 70, 260)
GUIDES = ["self", "u8", "f32"]          # the image guides itself; a separate uint8 guide (3 planes); a separate f32 guide (1 plane)
LAUNCHES = ["var_tails_x", "var_carry", "var_pass2_x", "var_tails_y", "var_carry", "var_pass2_y"]


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def guide_of(shape, kind):
    """the separate guide of a case, (C', H, W), or None"""
    if kind == "u8":
        return sc.byte_image((3,) + shape[1:], "guide")
    if kind == "f32":
        return sc.float_image((1,) + shape[1:], "guide")
    return None


def make_plan(shape, image, guide, K, sigma_s=S, sigma_r=R):
    import torch
    to_torch = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32}
    return rfa.SmoothPlan(shape[1:], planes=shape[0], guide_planes=0 if guide is None else guide.shape[0], image_dtype=to_torch[image.dtype],
                          guide_dtype=None if guide is None else to_torch[guide.dtype], iterations=K, sigma_s=sigma_s, sigma_r=sigma_r)


def run_plan(shape, image, guide, K, inplace=False, **sigmas):
    """(result on the host, the plan's bases)"""
    import torch
    with make_plan(shape, image, guide, K, **sigmas) as plan:
        src = dev(image)
        out = plan.execute(src, None if guide is None else dev(guide), src if inplace else None)
        torch.cuda.synchronize()
        return out.cpu().numpy(), [np.float32(b) for b in plan.bases]


def library_distances(image, guide):
    import torch
    dx, dy = rfa.domain_transform_distances(dev(image if guide is None else guide), S, R)
    torch.cuda.synchronize()
    return [dx.cpu().numpy(), dy.cpu().numpy()]


@functools.lru_cache(maxsize=None)
def library_bases(K):
    with rfa.SmoothPlan((40, 64), iterations=K, sigma_s=S, sigma_r=R, device=capi.RF_DEVICE_HOST_ONLY) as plan:
        return [np.float32(b) for b in plan.bases]


@functools.lru_cache(maxsize=None)
def expected(shape, image_kind, guide_kind, K):
    """(image, guide, f64 truth, the f32 serial loop's max abs error) on the distance planes and the bases the library reports:
    computed once, shared and never written"""
    image = sc.byte_image(shape) if image_kind == "u8" else sc.float_image(shape)
    guide = guide_of(shape, guide_kind)
    want, _, abs_err32 = sc.truth_and_yardstick(image, library_distances(image, guide), library_bases(K))
    want.setflags(write=False)
    return image, guide, want, abs_err32


# ---- f32 images: the launches of rf_var_distances and rf_var_plan_execute_power, bit for bit ---------------------------------
@pytest.mark.parametrize("guide_kind", GUIDES)
@pytest.mark.parametrize("shape", sc.SHAPES, ids=str)
def test_f32_equals_the_calls_written_out(shape, guide_kind):
    import torch
    K = 3
    C, H, W = shape
    image, guide = sc.float_image(shape), guide_of(shape, guide_kind)
    got, bases = run_plan(shape, image, guide, K)
    dx, dy = rfa.domain_transform_distances(dev(image if guide is None else guide), S, R)
    src = [t.contiguous() for t in dev(image)]
    with rfa.VarPlan((H, W), sc.SCANS, planes=C, n_weights=2) as plan:
        for a in bases:
            src = plan.execute_power(src, [dx, dy], [a, a])
        torch.cuda.synchronize()
    guarded.assert_bits_equal([torch.from_numpy(got[c]) for c in range(C)], [t.cpu() for t in src],
                              f"SmoothPlan {shape} guide {guide_kind} against rf_var_distances + {K} x execute_power")
    assert bases == library_bases(K)


@pytest.mark.parametrize("guide_kind", GUIDES)
def test_form_plan_agrees_with_form_power_on_f32(guide_kind):
    import torch
    shape, K = (3, 130, 132), 3
    image, guide, want, abs_err32 = expected(shape, "f32", guide_kind, K)
    g = None if guide is None else dev(guide)
    peak = float(np.max(np.abs(image)))
    for form in ("plan", "power"):
        got = rfa.edge_aware_smooth(dev(image), guide=g, sigma_s=S, sigma_r=R, iterations=K, form=form)
        torch.cuda.synchronize()
        assert got.dtype == torch.float32
        assert sc.f32_bar_excess(got.cpu().numpy(), want, abs_err32, peak, f'form="{form}" {shape} guide {guide_kind}') <= 0
    one = rfa.edge_aware_smooth(dev(image)[0], guide=dev(image), sigma_s=S, sigma_r=R, iterations=K, form="plan")      # (H, W)
    torch.cuda.synchronize()
    assert tuple(one.shape) == shape[1:]


# ---- byte images: the one-rounding rule --------------------------------------------------------------------------------------
BYTE_CASES = [(s, K) for s in sc.SHAPES[:2] for K in (1, 3)] + [(s, 3) for s in sc.SHAPES[2:]]


@pytest.mark.parametrize("guide_kind", GUIDES)
@pytest.mark.parametrize("shape,K", BYTE_CASES, ids=lambda v: str(v))
def test_bytes_under_the_one_rounding_rule(shape, K, guide_kind):
    image, guide, want, abs_err32 = expected(shape, "u8", guide_kind, K)
    got, bases = run_plan(shape, image, guide, K)
    assert bases == library_bases(K)
    assert sc.byte_rule_excess(got, want, abs_err32, f"bytes {shape} K = {K} guide {guide_kind}") <= 0
    assert (got != image).mean() > 0.5, "the filter left the image"


def test_form_plan_returns_bytes_for_bytes():
    import torch
    shape, K = (3, 130, 132), 3
    image, _, want, abs_err32 = expected(shape, "u8", "self", K)
    got = rfa.edge_aware_smooth(dev(image), sigma_s=S, sigma_r=R, iterations=K, form="plan")
    again = rfa.edge_aware_smooth(dev(image), sigma_s=S, sigma_r=R, iterations=K, form="plan")      # the cached plan
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape
    assert sc.byte_rule_excess(got.cpu().numpy(), want, abs_err32, 'form="plan" on bytes') <= 0
    assert guarded.bits_equal(got.cpu(), again.cpu())


# ---- exact cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0, 1, 137, 255])
def test_constant_byte_image_returns_itself(value):
    image = np.full(EXACT, value, dtype=np.uint8)
    got, _ = run_plan(EXACT, image, None, 3)
    np.testing.assert_array_equal(got, image)


@pytest.mark.parametrize("image_kind", ["u8", "f32"])
def test_checkerboard_guide_leaves_the_image(image_kind):
    """a 0 / 255 checkerboard with sigma_r = 1e-3: every distance is above 40000 and every weight underflows to exactly 0"""
    _, H, W = EXACT
    board = (255 * ((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2)).astype(np.uint8)[None]
    image = sc.byte_image(EXACT) if image_kind == "u8" else (sc.float_image(EXACT) * 2 - 1).astype(np.float32)
    got, _ = run_plan(EXACT, image, board, 3, sigma_s=40.0, sigma_r=1e-3)
    assert got.dtype == image.dtype
    np.testing.assert_array_equal(got.view(np.uint8), image.view(np.uint8))


# ---- in place and state ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guide_kind", ["self", "u8"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("image_kind", ["u8", "f32"])
def test_in_place_equals_out_of_place(image_kind, K, guide_kind):
    shape = (3, 130, 132)
    image = sc.byte_image(shape) if image_kind == "u8" else sc.float_image(shape)
    guide = guide_of(shape, guide_kind)
    a, _ = run_plan(shape, image, guide, K)
    b, _ = run_plan(shape, image, guide, K, inplace=True)
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


def test_no_state_is_kept_and_two_plans_live_together():
    import torch
    shape, K = EXACT, 3
    img8, other8 = sc.byte_image(shape), sc.byte_image(shape, "another image")
    img32, other32 = sc.float_image(shape), sc.float_image(shape, "another image")
    with make_plan(shape, img8, None, K) as p8, make_plan(shape, img32, None, K) as p32:
        first8, first32 = p8.execute(dev(img8)), p32.execute(dev(img32))
        mid8, mid32 = p8.execute(dev(other8)), p32.execute(dev(other32))
        third8, third32 = p8.execute(dev(img8)), p32.execute(dev(img32))
        torch.cuda.synchronize()
        assert guarded.bits_equal(third8.cpu(), first8.cpu()) and guarded.bits_equal(third32.cpu(), first32.cpu())
        assert not guarded.bits_equal(mid8.cpu(), first8.cpu()) and not guarded.bits_equal(mid32.cpu(), first32.cpu())
    alone8, _ = run_plan(shape, img8, None, K)
    alone32, _ = run_plan(shape, img32, None, K)
    np.testing.assert_array_equal(first8.cpu().numpy(), alone8)
    np.testing.assert_array_equal(first32.cpu().numpy().view(np.uint32), alone32.view(np.uint32))


# ---- guarded planes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_kind", ["u8", "f32"])
@pytest.mark.parametrize("shape", [(1, 70, 260), (3, 130, 132)], ids=str)
def test_guarded_planes(shape, image_kind):
    """Guards of 0xFF around image and guide (NaN in f32; for bytes a second run with 0x00 guards, bit-identical: the clamped
    loads of partial tiles are selected away), guards of 0xA5 around the output"""
    import torch
    K = 3
    C, H, W = shape
    image, guide, want, abs_err32 = expected(shape, image_kind, "u8", K)
    results = []
    for fill in (guarded.IN_FILL, guarded.IN_FILL_ZERO):
        d_in, g_in = guarded.guarded_planes((H, W), image.dtype, C, fill=fill)
        d_g, g_g = guarded.guarded_planes((H, W), np.uint8, guide.shape[0], fill=fill)
        d_out, g_out = guarded.guarded_planes((H, W), image.dtype, C, fill=guarded.OUT_FILL)
        g_in.load([torch.from_numpy(np.array(p)) for p in image])
        g_g.load([torch.from_numpy(np.array(p)) for p in guide])
        g_in.snapshot()
        g_g.snapshot()
        with make_plan(shape, image, guide, K) as plan:
            plan.execute(d_in, d_g, d_out)
            torch.cuda.synchronize()
        g_out.check_guards("output")
        g_in.check_unchanged("image")
        g_g.check_unchanged("guide")
        results.append([t.clone().cpu() for t in d_out])
    got = np.stack([t.numpy() for t in results[0]])
    if image_kind == "u8":
        assert sc.byte_rule_excess(got, want, abs_err32, f"guarded bytes {shape}") <= 0
    else:
        assert sc.f32_bar_excess(got, want, abs_err32, float(np.max(np.abs(image))), f"guarded f32 {shape}") <= 0
    guarded.assert_bits_equal(results[1], results[0], "guards of 0x00 against 0xFF")


# ---- timed execute -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_kind", ["u8", "f32"])
@pytest.mark.parametrize("K", [1, 3])
def test_timed_names_the_launch_list(K, image_kind):
    import torch
    shape = (1, 40, 64)
    image = sc.byte_image(shape) if image_kind == "u8" else sc.float_image(shape)
    plain, _ = run_plan(shape, image, None, K)
    with make_plan(shape, image, None, K) as plan:
        out, timed = plan.execute_timed(dev(image))
        torch.cuda.synchronize()
        assert [n for n, _ in timed] == ["var_distances"] + LAUNCHES * K
        assert len(timed) == plan.num_kernels == 1 + 6 * K
        assert all(ms >= 0 for _, ms in timed)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint8), plain.view(np.uint8))


# ---- refusals at execute -----------------------------------------------------------------------------------------------------
def raw_execute(plan, images, guides, outs):
    arr = lambda ptrs: None if ptrs is None else (ctypes.c_void_p * len(ptrs))(*ptrs)      # noqa: E731
    status = capi.lib().rf_smooth_plan_execute(plan._h, arr(images), arr(guides), arr(outs), None)
    return status, capi.lib().rf_last_error_string().decode()


def test_execute_refusals_on_a_device_plan():
    import torch
    H, W = 40, 64
    INVALID = capi.RF_ERR_INVALID_ARG
    b = torch.zeros((5, H, W), dtype=torch.uint8, device="cuda")
    f = torch.zeros((5, H, W), dtype=torch.float32, device="cuda")
    bp, fp = [b[i].data_ptr() for i in range(5)], [f[i].data_ptr() for i in range(5)]
    with rfa.SmoothPlan((H, W), planes=2, image_dtype=torch.uint8) as p8, rfa.SmoothPlan((H, W), planes=2) as p32, \
            rfa.SmoothPlan((H, W), planes=1, guide_planes=1, guide_dtype=torch.uint8) as guided:
        cases = [
            ("byte input off by 2", p8, ([bp[0] + 2, bp[1]], None, [bp[2], bp[3]])),
            ("byte output off by 2", p8, ([bp[0], bp[1]], None, [bp[2], bp[3] + 2])),
            ("f32 input off by 4", p32, ([fp[0] + 4, fp[1]], None, [fp[2], fp[3]])),
            ("f32 output off by 4", p32, ([fp[0], fp[1]], None, [fp[2] + 4, fp[3]])),
            ("byte input 0 is output 1", p8, ([bp[0], bp[1]], None, [bp[2], bp[0]])),
            ("f32 input 1 is output 0", p32, ([fp[0], fp[1]], None, [fp[1], fp[3]])),
            ("f32 input 16 bytes into output 0", p32, ([fp[2] + 16, fp[1]], None, [fp[2], fp[4]])),
            ("a guide for a self-guided plan", p8, ([bp[0], bp[1]], [bp[4]], [bp[2], bp[3]])),
            ("no guide for a guided plan", guided, ([fp[0]], None, [fp[1]])),
            ("uint8 guide off by 2", guided, ([fp[0]], [bp[0] + 2], [fp[1]])),
            ("null image plane", p8, ([bp[0], None], None, [bp[2], bp[3]])),
        ]
        for what, plan, args in cases:
            status, message = raw_execute(plan, *args)
            assert status == INVALID, f"{what}: status {status} ({message})"
            assert message, f"{what}: no text in rf_last_error_string"
        # what is allowed: in == out, and a guide plane that is an output plane
        assert raw_execute(p8, [bp[0], bp[1]], None, [bp[0], bp[1]])[0] == capi.RF_OK
        assert raw_execute(p32, [fp[0], fp[1]], None, [fp[0], fp[1]])[0] == capi.RF_OK
        assert raw_execute(guided, [fp[0]], [bp[0]], [fp[1]])[0] == capi.RF_OK
        torch.cuda.synchronize()
        with pytest.raises(TypeError):
            p8.execute(f[:2])
        with pytest.raises(ValueError):
            p8.execute(b[:3])
        with pytest.raises(ValueError):
            guided.execute(f[0])
        with pytest.raises(ValueError):
            p8.execute(b[:2], b[4])


def test_guide_may_be_the_output():
    """the distances are formed first, on the same stream: a byte image filtered onto its own separate guide"""
    import torch
    shape, K = EXACT, 3
    image, guide = sc.byte_image(shape), sc.byte_image(shape, "guide is out")
    apart, _ = run_plan(shape, image, guide, K)
    with make_plan(shape, image, guide, K) as plan:
        g = dev(guide)
        plan.execute(dev(image), g, g)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(g.cpu().numpy(), apart)


# ---- the whole filter --------------------------------------------------------------------------------------------------------
def test_edge_aware_smooth_of_a_byte_image():
    import torch
    image, clean = power.smooth_case()
    img8 = np.rint(255.0 * np.clip(image, 0.0, 1.0)).astype(np.uint8)
    got = rfa.edge_aware_smooth(dev(img8), sigma_s=40.0, sigma_r=0.5, iterations=3, form="plan")
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8
    power.assert_step_kept_noise_gone(image, clean, got.cpu().numpy().astype(np.float64) / 255.0, 'edge_aware_smooth, form="plan", bytes')


# ---- the C++ front-end -------------------------------------------------------------------------------------------------------
def test_cpp_frontend_smooth(tmp_path):
    """RecFilterSmooth on a 70 x 260 byte image against loops in the C++ file, under the byte rule; compiled here with the
    command line of test_cpp_frontend_varying_power"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_smooth.cpp")
    exe = str(tmp_path / "test_frontend_smooth")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "smooth-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
