"""Cases and the bar shared by tests/test_var_grad_host.py and tests/test_gpu_var_grad.py (a plain module: no fixtures).

Inputs and weights are those of tests/test_gpu_var_scans.py (`case`: weights with NaN at element 0 and a mean of 0.8); grad_out is
seeded, signed, in [-1, 1].  The bar, for the image gradient and for each weight gradient separately: max abs error against the f64
loops of tests/var_grad_loops.py over that gradient's f64 peak <= max(4 x the same figure of the f32 serial loops, 1e-6)."""
import functools
import zlib

import numpy as np

import var_grad_loops as loops
from test_gpu_var_scans import SCAN_LISTS, SHAPES, case      # noqa: F401  (re-exported)


@functools.lru_cache(maxsize=None)
def grad_out(shape, planes):
    rng = np.random.default_rng(zlib.crc32(repr(("grad_out", shape, planes)).encode()))
    g = [(rng.random(shape) * 2 - 1).astype(np.float32) for _ in range(planes)]
    for a in g:
        a.setflags(write=False)
    return g


def figures(got, want):
    """(max abs error / peak of `want`, peak) over a list of arrays"""
    peak = max(float(np.max(np.abs(w))) for w in want)
    err = max(float(np.max(np.abs(np.asarray(g, dtype=np.float64) - w))) for g, w in zip(got, want))
    return err / peak, peak


@functools.lru_cache(maxsize=None)
def expected(shape, planes, name, kind="uniform"):
    """f64 gradients and the f32 serial loops' error figures: (grad_ins, grad_weights, err32 of grad_ins, [err32 per weight plane])"""
    ins, ws = case(shape, planes, kind)
    g = grad_out(shape, planes)
    want_in, want_w = loops.backward(ins, ws, SCAN_LISTS[name], g, np.float64)
    ser_in, ser_w = loops.backward(ins, ws, SCAN_LISTS[name], g, np.float32)
    err_in = figures(ser_in, want_in)[0]
    err_w = [None if w is None else figures([s], [w])[0] for s, w in zip(ser_w, want_w)]
    return want_in, want_w, err_in, err_w


def assert_under_bar(got, want, err32, what):
    for g in got:
        assert not np.isnan(g).any(), f"{what}: NaN in the gradient"
    err, peak = figures(got, want)
    bar = max(4 * err32, 1e-6)
    print(f"{what}: err/peak {err:.3e}, f32 serial loops {err32:.3e}, ratio {err / max(err32, 1e-30):.2f}")
    assert err <= bar, f"{what}: err/peak {err:.3e} above the bar {bar:.3e} (f32 serial loops: {err32:.3e})"
    return err / max(err32, 1e-30)


def assert_gradients(got_in, got_w, shape, planes, name, what, kind="uniform"):
    """the image gradient and every weight gradient of a scan list under the bar; element 0 of a weight gradient exactly 0"""
    want_in, want_w, err_in, err_w = expected(shape, planes, name, kind)
    assert_under_bar(got_in, want_in, err_in, f"{what} grad_in")
    if got_w is None:
        return
    for k, (g, w, e) in enumerate(zip(got_w, want_w, err_w)):
        if w is None:
            continue
        assert_under_bar([g], [w], e, f"{what} grad_w[{k}]")
        first = g[:, 0] if k == 0 else g[0, :]      # plane 0 belongs to the x scans, plane 1 to the y scans
        assert np.array_equal(first, np.zeros_like(first)), f"{what} grad_w[{k}]: element 0 is not exactly 0"
