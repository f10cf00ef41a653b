"""Cases and the bar shared by tests/test_smooth_grad_host.py and tests/test_gpu_smooth_grad.py (a plain module: no fixtures).

Shapes, sigmas and images are those of tests/smooth_cases.py; grad_out is seeded and signed as tests/var_grad_cases.py's; guides
are seeded with no ties between neighbours (a ramp along x and along y under noise: the derivative of |.| is taken away from 0).
K = 2 everywhere, K = 1 and K = 3 on (1, 70, 260).  The bar, for every gradient (image, each exponent plane, guide) separately:
max abs error against the f64 loops of tests/smooth_grad_loops.py over that gradient's f64 peak <= max(4 x the same figure of the
f32 serial loops, 1e-6), no NaN (var_grad_cases.assert_under_bar)."""
import functools
import zlib

import numpy as np

import smooth_cases as sc
import smooth_grad_loops as sloops
import var_grad_cases as vcases

SHAPES = sc.SHAPES
SIGMA_S, SIGMA_R = sc.SIGMA_S, sc.SIGMA_R
SCALE = float(np.float32(SIGMA_S / SIGMA_R))      # what the plan hands var_distances for f32 guides
CASES = [(shape, 2) for shape in SHAPES] + [((1, 70, 260), 1), ((1, 70, 260), 3)]      # (shape, K)
figures, assert_under_bar = vcases.figures, vcases.assert_under_bar


def image(shape):
    return sc.float_image(shape)


@functools.lru_cache(maxsize=None)
def grad_out(shape):
    """(C, H, W), seeded, signed, in [-1, 1]"""
    g = np.stack(vcases.grad_out(tuple(shape[1:]), shape[0]))
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def guide(shape, channels=None):
    """seeded f32 guide of (channels, H, W) (default: the image's C) with no two neighbours equal, along x or along y"""
    C = shape[0] if channels is None else channels
    H, W = shape[1:]
    rng = np.random.default_rng(zlib.crc32(repr((shape, C, "smooth guide")).encode()))
    g = (0.5 * rng.random((C, H, W)) + np.linspace(0, 1, W)[None, None, :] + np.linspace(0, 1, H)[None, :, None]).astype(np.float32)
    assert (g[:, :, 1:] != g[:, :, :-1]).all() and (g[:, 1:, :] != g[:, :-1, :]).all(), "ties in the guide"
    g.setflags(write=False)
    return g


def bases(K):
    return sc.bases_f32(SIGMA_S, K)


@functools.lru_cache(maxsize=None)
def expected(shape, K, self_guided, edges):
    """f64 gradients and the f32 serial loops' error figures of the whole filter's backward:
    (grad_image, grad_guide or None, err32 of grad_image, err32 of grad_guide or None)"""
    gd = None if self_guided else guide(shape)
    want = sloops.smooth_backward(image(shape), gd, bases(K), SCALE, grad_out(shape), np.float64, edges)
    ser = sloops.smooth_backward(image(shape), gd, bases(K), SCALE, grad_out(shape), np.float32, edges)
    err_im = figures([ser[0]], [want[0]])[0]
    err_gd = None if want[1] is None else figures([ser[1]], [want[1]])[0]
    return want[0], want[1], err_im, err_gd


@functools.lru_cache(maxsize=None)
def exponent_planes(shape):
    """[d_x, d_y] (f32) of the shape's guide, by the f32 loops, NaN at element 0: what the power-form tests scan with"""
    d = sloops.distances(guide(shape), SCALE, np.float32)
    d[0][:, 0] = np.nan
    d[1][0, :] = np.nan
    for a in d:
        a.setflags(write=False)
    return d


POWER_BASES = [0.9, 0.8]      # of exponent plane 0 (x scans) and 1 (y scans)


@functools.lru_cache(maxsize=None)
def expected_power(shape, name):
    """f64 gradients of a scan list in the power form on the shape's image planes and exponent planes, and the f32 loops' figures:
    (grad_ins, grad_exponents, err32 of grad_ins, [err32 per exponent plane])"""
    planes, d, g = list(image(shape)), exponent_planes(shape), list(grad_out(shape))
    scans = vcases.SCAN_LISTS[name]
    want_in, want_d = sloops.power_backward(planes, d, POWER_BASES, scans, g, np.float64)
    ser_in, ser_d = sloops.power_backward(planes, d, POWER_BASES, scans, g, np.float32)
    err_in = figures(ser_in, want_in)[0]
    err_d = [None if w is None else figures([s], [w])[0] for s, w in zip(ser_d, want_d)]
    return want_in, want_d, err_in, err_d
