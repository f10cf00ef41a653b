"""Shapes, images, references and rules of the smoothing-plan tests (rf_smooth_plan_*, recfilter_amd.SmoothPlan): shared by
tests/test_smooth_host.py and tests/test_gpu_smooth.py; no tests here.

The filter: K iterations of +x -x +y -y (the serial loops of tests/test_gpu_var_scans.py) with weights 2^(d * log2 a_k) on two
distance planes d_x, d_y and the f32 bases a_k.  Truth is that in f64 (`weights_f64`), the yardstick the same loops in f32 fed
np.exp2(d * np.float32(log2 a_k)) (`weights_f32`), as tests/test_gpu_var_power.py::test_edge_aware_smooth_power has them.

The rules.
  f32 images   the project's bar: max abs error over the input peak <= max(4 x the f32 serial loop's, 1e-6).
  byte images  the one-rounding rule of tests/u8_cases.py, per sample, none left out:
                   |got - want64| <= 0.5 + 255 * max(4 * err32, 1e-6)
               0.5 is the one rounding to an integer (sat8: to nearest, ties to even); the rest is the f32 bar at the peak of a
               byte, err32 = the f32 serial loop's max abs error on the widened bytes over 255.  Derived, not measured."""
import functools
import zlib

import numpy as np

import test_gpu_var_scans as base            # the serial loops (the module, not its tests)

# (C, H, W): one tile each way; a partial last tile each way; three planes with a last x chunk 4 wide; 16 tiles along x;
# 16 tiles along y
SHAPES = [(1, 40, 64), (1, 70, 260), (3, 130, 132), (1, 8, 1024), (1, 1024, 8)]
SIGMA_S, SIGMA_R = 40.0, 0.5
SCANS = base.SCAN_LISTS["+x-x+y-y"]


# ---- images -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def byte_image(shape, what="image"):
    """seeded random bytes of (C, H, W); shared and never written"""
    rng = np.random.default_rng(zlib.crc32(repr((shape, what, "smooth bytes")).encode()))
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def float_image(shape, what="image"):
    """seeded f32 samples in [0, 1) of (C, H, W); shared and never written"""
    rng = np.random.default_rng(zlib.crc32(repr((shape, what, "smooth floats")).encode()))
    img = rng.random(shape).astype(np.float32)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def step_plus_noise_bytes(shape):
    """a step along x of 60 -> 190 with uniform noise of +-20, (C, H, W) bytes: edges to keep and noise to smooth"""
    rng = np.random.default_rng(zlib.crc32(repr((shape, "step")).encode()))
    W = shape[2]
    step = np.where(np.arange(W) < W // 2, 60, 190)
    img = np.clip(step[None, None, :] + rng.integers(-20, 21, size=shape), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


# ---- the filter in numpy ------------------------------------------------------------------------------------------------------
def bases_f32(sigma_s, K):
    """what rf_smooth_plan_bases reports, from the closed form: a_k rounded to f32"""
    import recfilter_amd as rfa
    return [np.float32(a) for a in rfa.domain_transform_bases(sigma_s, K)]


def distances_f32(guide, scale):
    """the formula of rf_var_distances on a (C, H, W) guide, in f64, rounded to f32 (the CPU tests' planes; the GPU tests take the
    library's own)"""
    g = np.asarray(guide, dtype=np.float64)
    dx = np.ones(g.shape[1:])
    dy = np.ones(g.shape[1:])
    dx[:, 1:] += scale * np.abs(g[:, :, 1:] - g[:, :, :-1]).sum(0)
    dy[1:, :] += scale * np.abs(g[:, 1:, :] - g[:, :-1, :]).sum(0)
    return [dx.astype(np.float32), dy.astype(np.float32)]


def weights_f64(d, a):
    return np.exp2(d.astype(np.float64) * np.log2(np.float64(np.float32(a))))


def weights_f32(d, a):
    w = np.exp2(d * np.float32(np.log2(np.float64(np.float32(a)))))
    assert w.dtype == np.float32
    return w


def sat8(v):
    """pixel.h: to nearest, ties to even; clamped to [0, 255]; NaN -> 0"""
    r = np.rint(np.asarray(v))
    return np.where(np.isnan(r), 0, np.clip(r, 0, 255)).astype(np.uint8)


def filter_loops(image, ds, bases, dtype, round_between=False):
    """K iterations of the serial loops on the planes of a (C, H, W) image in `dtype`; round_between: every iteration's result
    goes through bytes (the defect the byte rule must catch)"""
    conv = weights_f64 if dtype == np.float64 else weights_f32
    planes = [np.asarray(p, dtype=dtype) for p in image]
    for k, a in enumerate(bases):
        planes = base.reference(planes, [conv(d, a) for d in ds], SCANS, dtype)
        if round_between and k + 1 < len(bases):
            planes = [sat8(p).astype(dtype) for p in planes]
    return np.stack(planes)


def truth_and_yardstick(image, ds, bases):
    """(f64 truth, f32 serial loop, the serial loop's max abs error) of a (C, H, W) image, f32 or bytes (widened exactly)"""
    want = filter_loops(image, ds, bases, np.float64)
    serial = filter_loops(image, ds, bases, np.float32)
    return want, serial, float(np.max(np.abs(serial.astype(np.float64) - want)))


# ---- the rules ----------------------------------------------------------------------------------------------------------------
def f32_bar_excess(got, want, abs_err32, peak, what):
    """err / peak of `got` minus the bar max(4 * err32, 1e-6): the bar holds where this is <= 0"""
    assert got.dtype == np.float32 and not np.isnan(got).any(), f"{what}: NaN, or not f32"
    err, err32 = float(np.max(np.abs(got.astype(np.float64) - want))) / peak, abs_err32 / peak
    print(f"{what}: err/peak {err:.3e}, f32 serial loop {err32:.3e}, ratio {err / max(err32, 1e-30):.2f}")
    return err - max(4 * err32, 1e-6)


def byte_rule_excess(got, want, abs_err32, what):
    """max over all samples of |got - want64| minus (0.5 + 255 * max(4 * err32, 1e-6)): the rule holds where this is <= 0"""
    assert got.dtype == np.uint8 and got.shape == want.shape, f"{what}: not bytes of the image's shape"
    err32 = abs_err32 / 255.0
    bound = 0.5 + 255.0 * max(4 * err32, 1e-6)
    worst = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"{what}: max |got - want64| {worst:.6f}, bound {bound:.6f} (f32 serial loop over 255: {err32:.3e})")
    return worst - bound
