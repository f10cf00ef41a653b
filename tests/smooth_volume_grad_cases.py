"""Cases and the bar shared by tests/test_smooth_volume_grad_host.py and tests/test_gpu_smooth_volume_grad.py (a plain module: no
fixtures).

Shapes (C, D, H, W): (3, 20, 66, 68) -- partial tiles along x and y, three planes, two z segments of the distance kernels -- and
(1, 70, 8, 16) -- a partial z tile, five segments.  K = 2 on both, K = 1 and K = 3 on the second.  The distance adjoint alone also
runs on (16, 33, 5, 8) (16 channels, odd depth), (1, 1, 40, 64) (depth 1: gdz reaches nothing) and (2, 3, 1, 4) (one row, one
chunk).  Images are tests/smooth_cases.py's, grad_out and the distance gradients are seeded and signed as tests/var_grad_cases.py's,
guides are seeded with no ties between neighbours along any of the three axes (a ramp along x, y and z under noise: the derivative
of |.| is taken away from 0; the guide is f32 data, so the sign of a difference is the same in f32 and in f64).  spacing_z = 2.5.
The bar, for every gradient separately: max abs error against the f64 loops of tests/smooth_volume_grad_loops.py over that
gradient's f64 peak <= max(4 x the same figure of the f32 serial loops, 1e-6), no NaN (var_grad_cases.assert_under_bar)."""
import functools
import zlib

import numpy as np

import smooth_cases as sc
import smooth_volume_grad_loops as vsloops
import var_grad_cases as vcases

SHAPES = [(3, 20, 66, 68), (1, 70, 8, 16)]
CASES = [(SHAPES[0], 2), (SHAPES[1], 2), (SHAPES[1], 1), (SHAPES[1], 3)]      # (shape, K)
DISTANCE_SHAPES = SHAPES + [(16, 33, 5, 8), (1, 1, 40, 64), (2, 3, 1, 4)]
SIGMA_S, SIGMA_R, SPACING_Z = sc.SIGMA_S, sc.SIGMA_R, 2.5
SCALE = float(np.float32(SIGMA_S / SIGMA_R))                # what the plan hands the distance kernels for f32 guides
SCALE_U8 = float(np.float32(SIGMA_S / SIGMA_R / 255.0))     # and for byte guides
BYTE_GUIDE_CHANNELS = 3
figures, assert_under_bar = vcases.figures, vcases.assert_under_bar


def image(shape):
    return sc.float_image(shape)


@functools.lru_cache(maxsize=None)
def grad_out(shape):
    """(C, D, H, W), seeded, signed, in [-1, 1]"""
    g = np.stack(vcases.grad_out(tuple(shape[1:]), shape[0]))
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def guide(shape, channels=None):
    """seeded f32 guide of (channels, D, H, W) (default: the volume's C) with no two neighbours equal along x, y or z"""
    C = shape[0] if channels is None else channels
    D, H, W = shape[1:]
    rng = np.random.default_rng(zlib.crc32(repr((shape, C, "smooth volume guide")).encode()))
    g = (0.5 * rng.random((C, D, H, W)) + np.linspace(0, 1, W)[None, None, None, :] + np.linspace(0, 1, H)[None, None, :, None]
         + np.linspace(0, 1, D)[None, :, None, None]).astype(np.float32)
    assert (g[:, :, :, 1:] != g[:, :, :, :-1]).all() and (g[:, :, 1:, :] != g[:, :, :-1, :]).all() and (g[:, 1:] != g[:, :-1]).all(), "ties in the guide"
    g.setflags(write=False)
    return g


def byte_guide(shape):
    return sc.byte_image((BYTE_GUIDE_CHANNELS,) + tuple(shape[1:]), "guide")


def bases(K):
    return sc.bases_f32(SIGMA_S, K)


@functools.lru_cache(maxsize=None)
def distance_gradients(shape):
    """[gdx, gdy, gdz] of (D, H, W), seeded, signed, in [-1, 1]"""
    return vcases.grad_out(tuple(shape[1:]), 3)


@functools.lru_cache(maxsize=None)
def accumulate_pattern(shape):
    """what the gradient volumes hold before an accumulating call: (C, D, H, W), seeded, signed"""
    rng = np.random.default_rng(zlib.crc32(repr((shape, "accumulate")).encode()))
    p = (rng.random(shape) * 2 - 1).astype(np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def expected_distances(shape):
    """the distance adjoint on guide(shape): (f64 gradient, err32 of the f32 loops, f64 old + gradient, err32 of the f32 sum)"""
    gd = distance_gradients(shape)
    want = vsloops.distances_backward(guide(shape), SCALE, gd[0], gd[1], gd[2], np.float64)
    serial = vsloops.distances_backward(guide(shape), SCALE, gd[0], gd[1], gd[2], np.float32)
    old = accumulate_pattern(shape)
    want_sum = old.astype(np.float64) + want
    for a in (want, want_sum):
        a.setflags(write=False)
    return want, figures([serial], [want])[0], want_sum, figures([old + serial], [want_sum])[0]


@functools.lru_cache(maxsize=None)
def expected(shape, K, guide_kind, edges):
    """f64 gradients and the f32 serial loops' error figures of the whole filter's backward, guide_kind "self", "f32" or "u8" (a byte
    guide, taken as it is with the scale over 255; edges = 0 only):
    (grad_image, grad_guide or None, err32 of grad_image, err32 of grad_guide or None)"""
    gd, scale = {"self": (None, SCALE), "f32": (guide(shape), SCALE), "u8": (byte_guide(shape), SCALE_U8)}[guide_kind]
    assert guide_kind != "u8" or not edges
    want = vsloops.smooth_backward(image(shape), gd, bases(K), scale, SPACING_Z, grad_out(shape), np.float64, edges)
    ser = vsloops.smooth_backward(image(shape), gd, bases(K), scale, SPACING_Z, grad_out(shape), np.float32, edges)
    err_im = figures([ser[0]], [want[0]])[0]
    err_gd = None if want[1] is None else figures([ser[1]], [want[1]])[0]
    return want[0], want[1], err_im, err_gd


def expected_names(K, edges):
    """the launch list of rf_smooth_plan_backward on a volume plan with RF_SMOOTH_VOLUME_BACKWARD: 1 + 18 K, or 51 K - 7"""
    fwd, fwd_scans, adj = [], [], []
    for axis in "xyz":
        fwd += [f"var_tails_{axis}", "var_carry", f"var_pass2_{axis}"]
    for axis in "xxyyzz":
        fwd_scans += [f"var_tails_{axis}", "var_carry", f"var_pass2_{axis}"]
    for axis in "zzyyxx":
        adj += [f"var_adj_tails_{axis}", "var_carry", f"var_adj_pass2_{axis}"] + ([f"var_grad_{axis}"] if edges else [])
    if not edges:
        return ["var_distances_volume"] + adj * K
    return ["var_distances_volume"] + fwd * (K - 1) + (fwd_scans + adj) * K + ["var_distances_volume_grad"]
