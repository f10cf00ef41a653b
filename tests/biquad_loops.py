"""Serial loops of the time-varying direct-form-I section (rf_var2_plan_execute_biquad / _backward_biquad), the yardsticks of
tests/test_biquad_host.py and tests/test_gpu_biquad_signal.py, in the arithmetic of `dtype` (np.float64: the reference; np.float32:
the serial f32 loop the bar is measured against).  Arrays are (N,) or (L, N).  Built on tests/var2_loops.py:

    causal      v[n] = b0[n] x[n] + b1~[n] x[n-1] + b2~[n] x[n-2]          y = var2_loops.forward(v, a1, a2)
    adjoint     lam, grad_a1, grad_a2 = var2_loops.adjoint(a1, a2, y, g)
                grad_x[n]  = b0[n] lam[n] + b1~[n+1] lam[n+1] + b2~[n+2] lam[n+2]
                grad_b0[n] = lam[n] x[n]      grad_b1[n] = lam[n] x[n-1]      grad_b2[n] = lam[n] x[n-2]

The anticausal section is the causal one on all signals reversed.  b1[0], b2[0], b2[1] are replaced by 0 through a select, like
a1[0], a2[0], a2[1]; their gradients are 0.  v is a vectorised expression, so the long case is var2_loops' segmented form on v."""
import numpy as np

import var2_loops as loops


def _reversed(*arrays):
    return [None if a is None else np.asarray(a)[..., ::-1] for a in arrays]


def shifted(x, k):
    """x[n - k] with zeros before the line"""
    out = np.zeros_like(x)
    out[..., k:] = x[..., :x.shape[-1] - k]
    return out


def ahead(x, k):
    """x[n + k] with zeros behind the line"""
    out = np.zeros_like(x)
    out[..., :x.shape[-1] - k] = x[..., k:]
    return out


def masked_taps(b0, b1, b2, dtype):
    """(b0, b1~, b2~) of a causal section, in `dtype`"""
    b1, b2 = loops.masked(b1, b2, dtype)
    return np.asarray(b0, dtype=dtype), b1, b2


def feed_forward(x, b0, b1, b2, causal=True, dtype=np.float64):
    if not causal:
        return feed_forward(*_reversed(x, b0, b1, b2), True, dtype)[..., ::-1]
    x = np.asarray(x, dtype=dtype)
    b0, b1, b2 = masked_taps(b0, b1, b2, dtype)
    return b0 * x + b1 * shifted(x, 1) + b2 * shifted(x, 2)


def forward(x, b0, b1, b2, a1, a2, causal=True, dtype=np.float64):
    return loops.forward(feed_forward(x, b0, b1, b2, causal, dtype), a1, a2, causal, dtype)


def segmented_forward(x, b0, b1, b2, a1, a2, causal=True, dtype=np.float64):
    """`forward` on ONE long line whose a1, a2 cut it into segments"""
    return loops.segmented_forward(feed_forward(x, b0, b1, b2, causal, dtype), a1, a2, causal, dtype)


def tap_gradients(lam, x, b0, b1, b2, causal=True, dtype=np.float64):
    """(grad_x, grad_b0, grad_b1, grad_b2) from the adjoint state of the all-pole half: pointwise expressions"""
    if not causal:
        return tuple(r[..., ::-1] for r in tap_gradients(*_reversed(lam, x, b0, b1, b2), True, dtype))
    lam = np.asarray(lam, dtype=dtype)
    x = np.asarray(x, dtype=dtype)
    b0, b1, b2 = masked_taps(b0, b1, b2, dtype)
    gx = b0 * lam + ahead(b1 * lam, 1) + ahead(b2 * lam, 2)
    g1 = lam * shifted(x, 1)
    g2 = lam * shifted(x, 2)
    g1[..., :1] = 0
    g2[..., :2] = 0
    return gx, lam * x, g1, g2


def adjoint(x, b0, b1, b2, a1, a2, y, g, causal=True, dtype=np.float64):
    """(grad_x, grad_b0, grad_b1, grad_b2, grad_a1, grad_a2); y: the forward's output in `dtype`"""
    lam, ga1, ga2 = loops.adjoint(a1, a2, y, g, causal, dtype)
    return (*tap_gradients(lam, x, b0, b1, b2, causal, dtype), ga1, ga2)


def segmented_adjoint(x, b0, b1, b2, a1, a2, y, g, causal=True, dtype=np.float64):
    """`adjoint` on ONE long line"""
    lam, ga1, ga2 = loops.segmented_adjoint(a1, a2, y, g, causal, dtype)
    return (*tap_gradients(lam, x, b0, b1, b2, causal, dtype), ga1, ga2)
