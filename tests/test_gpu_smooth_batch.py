"""GPU tests of the batched smoothing plan (rf_smooth_plan_create_batched: the batch on gridDim.z of every kernel of
kernels_var.hip; recfilter_amd.SmoothPlan(batch=N), edge_aware_smooth on (N, C, H, W), RecFilterSmooth::batch).

No tolerance of its own: the single-image plan is held to the f64 loops by tests/test_gpu_smooth.py and
tests/test_gpu_smooth_grad.py, and the batched plan is held to the single-image plan BIT FOR BIT -- every image of a batch, forward
and backward, at every position, whatever its neighbours hold.  Every image has its own seeded content (smooth_cases.float_image /
byte_image with the image's index in the seed).  The single-image results are computed once per case and shared."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import guarded
import smooth_cases as sc
import recfilter_amd as rfa
from recfilter_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA_S, SIGMA_R = sc.SIGMA_S, sc.SIGMA_R
# one tile; partial tiles both ways; three planes; many tiles along x; many tiles along y
CASES = [(s, n) for s in [(1, 40, 64), (1, 70, 260), (3, 130, 132)] for n in (1, 2, 5)] + [((1, 8, 1024), 3), ((1, 1024, 8), 3)]
MID = (1, 70, 260)
G = 2      # planes of a separate guide


def torch_():
    import torch
    return torch


def host_batch(shape, n, dtype, what="image"):
    """(n, C, H, W) on the host: image b seeded by (shape, b)"""
    make = sc.byte_image if dtype == np.uint8 else sc.float_image
    return np.stack([make(shape, f"{what} {b}") for b in range(n)])


def guide_shape(shape):
    return (G,) + tuple(shape[1:])


def dev(a):
    return torch_().from_numpy(np.ascontiguousarray(a)).cuda()


def tdtype(dtype):
    return torch_().uint8 if dtype == np.uint8 else torch_().float32


def plan_of(shape, dtype, guide_dtype, K, batch=None):
    return rfa.SmoothPlan(shape[1:], planes=shape[0], guide_planes=0 if guide_dtype is None else G, image_dtype=tdtype(dtype),
                          guide_dtype=None if guide_dtype is None else tdtype(guide_dtype), iterations=K, sigma_s=SIGMA_S, sigma_r=SIGMA_R,
                          batch=batch)


@functools.lru_cache(maxsize=None)
def singles_forward(shape, n, dtype, guide_dtype, K):
    """the single-image plan's outputs of images 0 .. n-1, stacked (a device tensor; shared, never written)"""
    torch = torch_()
    img = dev(host_batch(shape, n, dtype))
    gd = None if guide_dtype is None else dev(host_batch(guide_shape(shape), n, guide_dtype, "guide"))
    with plan_of(shape, dtype, guide_dtype, K) as one:
        out = torch.stack([one.execute(img[b], None if gd is None else gd[b]) for b in range(n)])
        torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def singles_backward(shape, n, separate, edges):
    """the single-image plan's (grad_image, grad_guide or None) of images 0 .. n-1, stacked"""
    torch = torch_()
    img, go = dev(host_batch(shape, n, np.float32)), dev(host_batch(shape, n, np.float32, "grad_out"))
    gd = dev(host_batch(guide_shape(shape), n, np.float32, "guide")) if separate else None
    gi, gg = [], []
    with plan_of(shape, np.float32, np.float32 if separate else None, 2) as one:
        for b in range(n):
            a, c = one.backward(img[b], None if gd is None else gd[b], go[b], edges=edges)
            gi.append(a)
            gg.append(c)
        torch.cuda.synchronize()
    return torch.stack(gi), torch.stack(gg) if gg[0] is not None else None


def assert_same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    for b in range(got.shape[0]):
        assert guarded.bits_equal(got[b], want[b]), f"{what}: image {b} of {got.shape[0]} differs from the single-image plan's"


# ---- forward --------------------------------------------------------------------------------------------------------------------
FORWARD = [(s, n, dt, g, 2) for s, n in CASES for dt, g in ((np.float32, None), (np.float32, np.float32), (np.uint8, None), (np.uint8, np.float32))] + \
          [(MID, n, np.uint8, np.uint8, 2) for n in (1, 2, 5)] + [(MID, n, np.float32, np.uint8, 2) for n in (2,)] + \
          [(MID, n, dt, g, K) for n in (1, 2, 5) for K in (1, 3) for dt, g in ((np.float32, None), (np.float32, np.float32), (np.uint8, None))]


def _fid(c):
    s, n, dt, g, K = c
    return f"{n}x{s[0]}x{s[1]}x{s[2]}-{np.dtype(dt).name}-{'self' if g is None else 'guide_' + np.dtype(g).name}-K{K}"


@pytest.mark.parametrize("case", FORWARD, ids=[_fid(c) for c in FORWARD])
def test_forward_equals_the_single_image_plan(case):
    shape, n, dtype, guide_dtype, K = case
    torch = torch_()
    want = singles_forward(shape, n, dtype, guide_dtype, K)
    img = dev(host_batch(shape, n, dtype))
    gd = None if guide_dtype is None else dev(host_batch(guide_shape(shape), n, guide_dtype, "guide"))
    with plan_of(shape, dtype, guide_dtype, K, batch=n) as plan:
        assert plan.batch == n and plan.num_kernels == 1 + 6 * K
        keep = img.clone()
        out = plan.execute(img, gd)
        torch.cuda.synchronize()
        assert_same_bits(out, want, "out of place")
        assert torch.equal(img, keep), "an out-of-place execute wrote its input"
        again = plan.execute(img, gd, out=img)      # in place
        torch.cuda.synchronize()
        assert again is img
        assert_same_bits(img, want, "in place")


# ---- backward -------------------------------------------------------------------------------------------------------------------
BACKWARD = [(s, n, sep, e) for s, n in CASES for sep in (False, True) for e in (False, True)]


@pytest.mark.parametrize("case", BACKWARD, ids=[f"{n}x{s[0]}x{s[1]}x{s[2]}-{'guide' if sep else 'self'}-edges{int(e)}" for s, n, sep, e in BACKWARD])
def test_backward_equals_the_single_image_plan(case):
    shape, n, separate, edges = case
    torch = torch_()
    want_gi, want_gg = singles_backward(shape, n, separate, edges)
    img, go = dev(host_batch(shape, n, np.float32)), dev(host_batch(shape, n, np.float32, "grad_out"))
    gd = dev(host_batch(guide_shape(shape), n, np.float32, "guide")) if separate else None
    with plan_of(shape, np.float32, np.float32 if separate else None, 2, batch=n) as plan:
        assert plan.backward_num_kernels(edges) == (64 if edges else 25)
        gi, gg = plan.backward(img, gd, go, edges=edges)
        torch.cuda.synchronize()
        assert_same_bits(gi, want_gi, "grad_image")
        assert (gg is None) == (want_gg is None)
        if gg is not None:
            assert_same_bits(gg, want_gg, "grad_guide")
        # repeated: the same bits (poisoned destinations: everything is stored, nothing added to what was there)
        gi2, gg2 = plan.backward(img, gd, go, torch.full_like(go, np.nan), None if gg is None else torch.full_like(gd, np.nan), edges=edges)
        torch.cuda.synchronize()
        assert guarded.bits_equal(gi2, gi) and (gg is None or guarded.bits_equal(gg2, gg)), "a repeated backward gave other bits"
        # in place: grad_image is grad_out
        work = go.clone()
        gi3, _ = plan.backward(img, gd, work, work, edges=edges)
        torch.cuda.synchronize()
        assert gi3 is work and guarded.bits_equal(work, gi), "in place differs from out of place"


# ---- isolation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [MID, (3, 130, 132)], ids=str)
def test_a_nan_image_reaches_no_other_image(shape):
    torch = torch_()
    n = 3
    img, go = dev(host_batch(shape, n, np.float32)), dev(host_batch(shape, n, np.float32, "grad_out"))
    want = singles_forward(shape, n, np.float32, None, 2)
    want_gi, _ = singles_backward(shape, n, False, True)
    img[1] = float("nan")
    go_nan = go.clone()
    go_nan[1] = float("nan")
    with plan_of(shape, np.float32, None, 2, batch=n) as plan:
        out = plan.execute(img)
        gi, _ = plan.backward(img, None, go_nan, edges=True)
        torch.cuda.synchronize()
    assert bool(torch.isnan(out[1]).all()) and bool(torch.isnan(gi[1]).any())
    for b in (0, 2):
        assert guarded.bits_equal(out[b], want[b]), f"forward: image {b} changed beside a NaN image"
        assert guarded.bits_equal(gi[b], want_gi[b]), f"backward: image {b} changed beside a NaN image"


@pytest.mark.parametrize("shape,n", [(MID, 5), ((3, 130, 132), 2), ((1, 8, 1024), 3), ((1, 1024, 8), 3)], ids=str)
def test_an_image_gives_the_same_bits_at_every_position(shape, n):
    """the batch reversed: image b now sits at position n-1-b (so image 0 at the end, image n-1 at the front)"""
    torch = torch_()
    img, go = dev(host_batch(shape, n, np.float32)), dev(host_batch(shape, n, np.float32, "grad_out"))
    want = singles_forward(shape, n, np.float32, None, 2)
    want_gi, _ = singles_backward(shape, n, False, True)
    with plan_of(shape, np.float32, None, 2, batch=n) as plan:
        out = plan.execute(img.flip(0).contiguous())
        gi, _ = plan.backward(img.flip(0).contiguous(), None, go.flip(0).contiguous(), edges=True)
        torch.cuda.synchronize()
    assert_same_bits(out.flip(0), want, "forward, reversed batch")
    assert_same_bits(gi.flip(0), want_gi, "backward, reversed batch")


# ---- strides above dense, through the C ABI ---------------------------------------------------------------------------------------
class RawPlan:
    """rf_smooth_plan_create_batched with strides of the caller's choice"""

    def __init__(self, shape, u8, n_guide, K, batch, image_stride, guide_stride):
        d = capi.SmoothDesc()
        d.abi, d.image_u8, d.width, d.height, d.n_planes, d.n_guide, d.guide_u8 = capi.RF_ABI, int(u8), shape[2], shape[1], shape[0], n_guide, 0
        d.iterations, d.sigma_s, d.sigma_r, d.device, d.flags = K, SIGMA_S, SIGMA_R, -1, 0
        b = capi.SmoothBatchDesc()
        b.batch, b.image_stride, b.guide_stride = batch, image_stride, guide_stride
        self.h = ctypes.c_void_p()
        capi.check(capi.lib().rf_smooth_plan_create_batched(ctypes.byref(d), ctypes.byref(b), ctypes.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        capi.lib().rf_smooth_plan_destroy(self.h)


def pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def padded(shape, n, dtype, fill):
    """n images of `shape` as n * C guarded planes of one allocation: (Guarded, samples from image to image, a multiple of 4 above
    the dense C*H*W).  Plane pl of image b is view b * C + pl; guards lie before, between and behind all of them."""
    C = shape[0]
    g = guarded.Guarded(shape[1:], dtype, n * C, fill=fill)
    itemsize = g.plane_bytes // (shape[1] * shape[2])
    pitch = g.offsets[1] - g.offsets[0] if n * C > 1 else 0
    assert (C * pitch) % (4 * itemsize) == 0 and C * pitch // itemsize > C * shape[1] * shape[2]
    return g, C * pitch // itemsize


def stream():
    return ctypes.c_void_p(torch_().cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "uint8"])
@pytest.mark.parametrize("shape,n", [(MID, 2), ((3, 130, 132), 2)], ids=str)
def test_strided_forward_stays_inside_its_planes(shape, n, dtype):
    torch = torch_()
    C = shape[0]
    want = singles_forward(shape, n, dtype, None, 2)
    src, stride = padded(shape, n, dtype, guarded.IN_FILL)      # (NaN between the planes of an f32 image: none may be loaded and used)
    dst, stride_out = padded(shape, n, dtype, guarded.OUT_FILL)
    assert stride == stride_out
    host = host_batch(shape, n, dtype)
    src.load([dev(host[b, pl]) for b in range(n) for pl in range(C)])
    src.snapshot()
    with RawPlan(shape, dtype == np.uint8, 0, 2, n, stride, 0) as plan:
        capi.check(capi.lib().rf_smooth_plan_execute(plan.h, pointers(src.views[:C]), None, pointers(dst.views[:C]), stream()))
        torch.cuda.synchronize()
    dst.check_guards("strided output")
    src.check_unchanged("strided input")
    got = torch.stack([torch.stack(dst.views[b * C:(b + 1) * C]) for b in range(n)])
    assert_same_bits(got, want, "strided forward")


@pytest.mark.parametrize("separate", [False, True], ids=["self", "guide"])
def test_strided_backward_stays_inside_its_planes(separate):
    torch = torch_()
    shape, n = (3, 130, 132), 2
    C = shape[0]
    want_gi, want_gg = singles_backward(shape, n, separate, True)
    roles = {"image": (shape, guarded.IN_FILL), "grad_out": (shape, guarded.IN_FILL), "grad_image": (shape, guarded.OUT_FILL)}
    if separate:
        roles.update({"guide": (guide_shape(shape), guarded.IN_FILL), "grad_guide": (guide_shape(shape), guarded.OUT_FILL)})
    mem, strides = {}, {}
    for role, (s, fill) in roles.items():
        mem[role], strides[role] = padded(s, n, np.float32, fill)
    for role in ("image", "grad_out", "guide"):
        if role in mem:
            s = roles[role][0]
            host = host_batch(s, n, np.float32, role)
            mem[role].load([dev(host[b, pl]) for b in range(n) for pl in range(s[0])])
            mem[role].snapshot()
    with RawPlan(shape, False, G if separate else 0, 2, n, strides["image"], strides["guide"] if separate else 0) as plan:
        capi.check(capi.lib().rf_smooth_plan_backward(
            plan.h, pointers(mem["image"].views[:C]), pointers(mem["guide"].views[:G]) if separate else None, pointers(mem["grad_out"].views[:C]),
            pointers(mem["grad_image"].views[:C]), pointers(mem["grad_guide"].views[:G]) if separate else None, 1, stream()))
        torch.cuda.synchronize()
    for role in mem:
        if role.startswith("grad_") and role != "grad_out":
            mem[role].check_guards(role)
        else:
            mem[role].check_unchanged(role)
    got = torch.stack([torch.stack(mem["grad_image"].views[b * C:(b + 1) * C]) for b in range(n)])
    assert_same_bits(got, want_gi, "strided grad_image")
    if separate:
        got = torch.stack([torch.stack(mem["grad_guide"].views[b * G:(b + 1) * G]) for b in range(n)])
        assert_same_bits(got, want_gg, "strided grad_guide")


def test_strides_that_break_the_rules_are_refused():
    torch = torch_()
    shape, n = (3, 40, 64), 2
    C, S = shape[0], shape[1] * shape[2]
    L = capi.lib()
    img, out = torch.zeros((n + 1, C, S), device="cuda"), torch.zeros((n + 1, C, S), device="cuda")
    planes = lambda t: pointers([t[0, c] for c in range(C)])      # noqa: E731
    # a stride that is not a multiple of 4 samples: no plan
    with pytest.raises(capi.RecFilterError, match="multiples of 4"):
        RawPlan(shape, False, 0, 2, n, C * S + 2, 0)
    # a stride of ONE plane where an image has three: image 1's plane 0 is image 0's plane 1
    with RawPlan(shape, False, 0, 2, n, S, 0) as plan:
        assert L.rf_smooth_plan_execute(plan.h, planes(img), None, planes(out), stream()) == capi.RF_ERR_INVALID_ARG
        message = L.rf_last_error_string().decode()
        assert "output plane" in message and "of image 1" in message and "of image 0" in message and "overlaps" in message, message
        # in place as well: image 1's input plane 0 is image 0's output plane 1
        assert L.rf_smooth_plan_execute(plan.h, planes(img), None, planes(img), stream()) == capi.RF_ERR_INVALID_ARG
    with RawPlan(shape, False, 0, 2, n, C * S, 0) as plan:
        # dense and disjoint, or exactly in place: fine
        capi.check(L.rf_smooth_plan_execute(plan.h, planes(img), None, planes(out), stream()))
        capi.check(L.rf_smooth_plan_execute(plan.h, planes(img), None, planes(img), stream()))
        # the output one plane further: out[b][pl] is image[b][pl + 1], and image 1's first plane image 0's last
        shifted = pointers([img[0, c] if c < C else img[1, 0] for c in range(1, C + 1)])
        assert L.rf_smooth_plan_execute(plan.h, planes(img), None, shifted, stream()) == capi.RF_ERR_INVALID_ARG
        message = L.rf_last_error_string().decode()
        assert "output plane" in message and "input plane" in message and "overlaps" in message, message
        # backward: grad_image on the image
        go = torch.zeros((n, C, S), device="cuda")
        assert L.rf_smooth_plan_backward(plan.h, planes(img), None, planes(go), planes(img), None, 0, stream()) == capi.RF_ERR_INVALID_ARG
        message = L.rf_last_error_string().decode()
        assert "grad_image plane" in message and "image plane" in message, message
        capi.check(L.rf_smooth_plan_backward(plan.h, planes(img), None, planes(go), planes(go), None, 0, stream()))      # in place: allowed
        torch.cuda.synchronize()


# ---- the launch list ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("separate", [False, True], ids=["self", "guide"])
def test_launch_lists_are_the_single_image_plans(separate):
    torch = torch_()
    shape, n, K = MID, 5, 2
    img, go = dev(host_batch(shape, n, np.float32)), dev(host_batch(shape, n, np.float32, "grad_out"))
    gd = dev(host_batch(guide_shape(shape), n, np.float32, "guide")) if separate else None
    guide_dtype = np.float32 if separate else None
    with plan_of(shape, np.float32, guide_dtype, K) as one, plan_of(shape, np.float32, guide_dtype, K, batch=n) as plan:
        _, t1 = one.execute_timed(img[0], None if gd is None else gd[0])
        out, tn = plan.execute_timed(img, gd)
        assert [name for name, _ in tn] == [name for name, _ in t1] and len(tn) == 1 + 6 * K
        assert_same_bits(out, singles_forward(shape, n, np.float32, guide_dtype, K), "execute_timed")
        for edges in (False, True):
            _, _, b1 = one.backward_timed(img[0], None if gd is None else gd[0], go[0], edges=edges)
            gi, gg, bn = plan.backward_timed(img, gd, go, edges=edges)
            assert [name for name, _ in bn] == [name for name, _ in b1] and len(bn) == (34 * K - 4 if edges else 1 + 12 * K)
            assert all(ms >= 0.0 for _, ms in bn)
            want_gi, want_gg = singles_backward(shape, n, separate, edges)
            assert_same_bits(gi, want_gi, "backward_timed")
            if want_gg is not None:
                assert_same_bits(gg, want_gg, "backward_timed, guide")
    torch.cuda.synchronize()


# ---- no state -------------------------------------------------------------------------------------------------------------------
def test_three_steps_interleaved_with_a_single_image_plan():
    torch = torch_()
    shape, n = (3, 130, 132), 2
    img, go = dev(host_batch(shape, n, np.float32)), dev(host_batch(shape, n, np.float32, "grad_out"))
    other = dev(host_batch(shape, n, np.float32, "another image"))
    with plan_of(shape, np.float32, None, 2) as one, plan_of(shape, np.float32, None, 2, batch=n) as plan:
        first = plan.execute(img).clone()
        first_g = plan.backward(img, None, go, edges=True)[0].clone()
        one_first = one.execute(img[1]).clone()
        plan.execute(other)                                        # another batch in between
        plan.backward(other, None, other, edges=True)
        one.execute(other[0])
        third = plan.execute(img)
        third_g = plan.backward(img, None, go, edges=True)[0]
        one_third = one.execute(img[1])
        torch.cuda.synchronize()
    assert guarded.bits_equal(first, third) and guarded.bits_equal(first_g, third_g), "the batched plan kept state across steps"
    assert guarded.bits_equal(one_first, one_third) and guarded.bits_equal(one_first, first[1])


# ---- autograd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["image", "guide", "self"])
def test_apply_and_edge_aware_smooth_match_the_per_image_calls(mode):
    """mode image: a separate guide that needs no gradient; guide: image and guide both; self: the image guides itself"""
    torch = torch_()
    shape, n, K = MID, 3, 2
    separate = mode != "self"

    def leaves():
        img = dev(host_batch(shape, n, np.float32)).requires_grad_(True)
        gd = dev(host_batch(guide_shape(shape), n, np.float32, "guide")).requires_grad_(mode == "guide") if separate else None
        return img, gd

    go = dev(host_batch(shape, n, np.float32, "grad_out"))
    # per image: 3-D calls
    img1, gd1 = leaves()
    outs = [rfa.edge_aware_smooth(img1[b], None if gd1 is None else gd1[b], SIGMA_S, SIGMA_R, K, form="plan", differentiable=True) for b in range(n)]
    want = torch.stack(outs)
    want.backward(go)
    # the batch, by the plan and by edge_aware_smooth
    for how in ("apply", "edge_aware_smooth"):
        img, gd = leaves()
        if how == "apply":
            with plan_of(shape, np.float32, np.float32 if separate else None, K, batch=n) as plan:
                out = plan.apply(img, gd)
                out.backward(go)
                torch.cuda.synchronize()
        else:
            out = rfa.edge_aware_smooth(img, gd, SIGMA_S, SIGMA_R, K, form="plan", differentiable=True)
            out.backward(go)
        assert out.grad_fn is not None and guarded.bits_equal(out.detach(), want.detach()), how
        assert guarded.bits_equal(img.grad, img1.grad), f"{how}: image gradient"
        if mode == "guide":
            assert guarded.bits_equal(gd.grad, gd1.grad), f"{how}: guide gradient"
        elif gd is not None:
            assert gd.grad is None
    # without the flag: no grad_fn; the other forms still refuse 4-D
    img, gd = leaves()
    plain = rfa.edge_aware_smooth(img, gd, SIGMA_S, SIGMA_R, K, form="plan")
    assert plain.grad_fn is None and guarded.bits_equal(plain, want.detach())
    with pytest.raises(ValueError):
        rfa.edge_aware_smooth(img.detach(), None, SIGMA_S, SIGMA_R, K, form="power")
    with pytest.raises(ValueError):
        rfa.edge_aware_smooth(img.detach(), None, SIGMA_S, SIGMA_R, K, form="planes")


def test_python_argument_checks():
    torch = torch_()
    shape, n = (1, 40, 64), 2
    img = dev(host_batch(shape, n, np.float32))
    with plan_of(shape, np.float32, None, 2, batch=n) as plan:
        with pytest.raises(ValueError):
            plan.execute(img[0])                                      # wrong rank
        with pytest.raises(ValueError):
            plan.execute(torch.cat([img, img]))                       # wrong N
        with pytest.raises(ValueError):
            plan.execute(torch.zeros((n, 1, 40, 128), device="cuda")[..., ::2])      # the right shape, not contiguous
        with pytest.raises(TypeError):
            plan.execute(img.to(torch.uint8))                         # wrong dtype
        with pytest.raises(ValueError):
            plan.execute(img, guide=img)                              # this plan's image guides itself
        with pytest.raises(ValueError):
            plan.backward(img, None, img[0])


# ---- the C++ front-end ----------------------------------------------------------------------------------------------------------
def test_cpp_frontend_smooth_batch(tmp_path):
    """RecFilterSmooth::batch(3, ...) against three single realizes and gradients, bit for bit; compiled here with the command
    line of test_gpu_smooth.py::test_cpp_frontend_smooth"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_smooth_batch.cpp")
    exe = str(tmp_path / "test_frontend_smooth_batch")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "smooth-batch-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
