"""Serial loops of the time-varying second-order all-pole scan (rf_var2_plan_*), the yardsticks of tests/test_var2_host.py and
tests/test_gpu_var2_signal.py, in the arithmetic of `dtype` (np.float64: the reference; np.float32: the serial f32 loop the bar
is measured against).  Arrays are (N,) or (L, N); the loops run over n and are vectorised over the lines.

    causal      y[n] = x[n] - a1~[n] y[n-1] - a2~[n] y[n-2]          anticausal: the causal scan on the three signals reversed
    adjoint     lam[n] = g[n] - a1~[n+1] lam[n+1] - a2~[n+2] lam[n+2],   grad_a1[n] = -lam[n] y[n-1],   grad_a2[n] = -lam[n] y[n-2]

a~: a1[0], a2[0], a2[1] replaced by 0 through a select (whatever they hold, a NaN included); their gradients are 0.

Long signals: where a1[n] = a2[n] = a2[n+1] = 0 the state decouples -- y[n] = x[n] and y[n+1] sees only y[n] -- so the line splits
into segments that run as the lines of one vectorised call (`segmented_forward`, `segmented_adjoint`)."""
import numpy as np


def masked(a1, a2, dtype):
    """(a1~, a2~) of a causal scan, in `dtype`"""
    a1 = np.array(a1, dtype=dtype)
    a2 = np.array(a2, dtype=dtype)
    a1[..., :1] = 0
    a2[..., :2] = 0
    return a1, a2


def _reversed(*arrays):
    return [None if a is None else np.asarray(a)[..., ::-1] for a in arrays]


def forward(x, a1, a2, causal=True, dtype=np.float64):
    if not causal:
        return forward(*_reversed(x, a1, a2), True, dtype)[..., ::-1]
    x = np.asarray(x, dtype=dtype)
    a1, a2 = masked(a1, a2, dtype)
    n = x.shape[-1]
    y = np.empty_like(x)
    y1 = np.zeros(x.shape[:-1], dtype=dtype)
    y2 = np.zeros(x.shape[:-1], dtype=dtype)
    for i in range(n):
        v = x[..., i] - a1[..., i] * y1 - a2[..., i] * y2
        y[..., i] = v
        y2, y1 = y1, v
    return y


def adjoint_state(a1, a2, g, causal=True, dtype=np.float64):
    """lam = dL/dx from g = dL/dy"""
    if not causal:
        return adjoint_state(*_reversed(a1, a2, g), True, dtype)[..., ::-1]
    g = np.asarray(g, dtype=dtype)
    a1, a2 = masked(a1, a2, dtype)
    n = g.shape[-1]
    lam = np.empty_like(g)
    l1 = np.zeros(g.shape[:-1], dtype=dtype)      # lam[i+1]
    l2 = np.zeros(g.shape[:-1], dtype=dtype)      # lam[i+2]
    zero = np.zeros(g.shape[:-1], dtype=dtype)
    for i in range(n - 1, -1, -1):
        c1 = a1[..., i + 1] if i + 1 < n else zero
        c2 = a2[..., i + 2] if i + 2 < n else zero
        v = g[..., i] - c1 * l1 - c2 * l2
        lam[..., i] = v
        l2, l1 = l1, v
    return lam


def coefficient_gradients(lam, y, causal=True, dtype=np.float64):
    """(grad_a1, grad_a2) from the adjoint state and the forward's output: one pointwise expression"""
    if not causal:
        g1, g2 = coefficient_gradients(*_reversed(lam, y), True, dtype)
        return g1[..., ::-1], g2[..., ::-1]
    lam = np.asarray(lam, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    g1 = np.zeros_like(lam)
    g2 = np.zeros_like(lam)
    g1[..., 1:] = -lam[..., 1:] * y[..., :-1]
    g2[..., 2:] = -lam[..., 2:] * y[..., :-2]
    return g1, g2


def adjoint(a1, a2, y, g, causal=True, dtype=np.float64):
    """(grad_x, grad_a1, grad_a2); y: the forward's output in `dtype`"""
    lam = adjoint_state(a1, a2, g, causal, dtype)
    return (lam, *coefficient_gradients(lam, y, causal, dtype))


# ---- the segmented form -----------------------------------------------------------------------------------------------------------
def segment_starts(a1, a2):
    """where a causal scan on one line decouples: 0, and every n with a1[n] = a2[n] = a2[n+1] = 0"""
    a1 = np.asarray(a1)
    a2 = np.asarray(a2)
    n = a1.shape[0]
    next_zero = np.append(a2[1:] == 0, True)
    cut = (a1 == 0) & (a2 == 0) & next_zero
    cut[0] = True
    return np.flatnonzero(cut)


def _gathered(starts, n, arrays, dtype):
    ends = np.append(starts[1:], n)
    width = int((ends - starts).max())
    at = starts[:, None] + np.arange(width)[None, :]
    inside = at < ends[:, None]
    at = np.minimum(at, n - 1)
    return at, inside, [np.where(inside, np.asarray(a)[at], 0).astype(dtype) for a in arrays]


def segmented_forward(x, a1, a2, causal=True, dtype=np.float64):
    """`forward` on ONE long line (N,), its segments as the lines of one vectorised call"""
    if not causal:
        return segmented_forward(*_reversed(x, a1, a2), True, dtype)[::-1]
    n = np.asarray(x).shape[0]
    a1m, a2m = masked(a1, a2, dtype)
    starts = segment_starts(a1m, a2m)
    at, inside, (xs, s1, s2) = _gathered(starts, n, [x, a1m, a2m], dtype)
    y = np.empty(n, dtype=dtype)
    y[at[inside]] = forward(xs, s1, s2, True, dtype)[inside]
    return y


def segmented_adjoint(a1, a2, y, g, causal=True, dtype=np.float64):
    """`adjoint` on ONE long line: lam inside a segment sees only lam inside it (the coefficients that would couple it to the next
    segment are the zeros that cut the line); the coefficient gradients are pointwise in lam and y over the whole line -- the
    gradient of a zero that cuts is not zero"""
    if not causal:
        return tuple(r[::-1] for r in segmented_adjoint(*_reversed(a1, a2, y, g), True, dtype))
    n = np.asarray(g).shape[0]
    a1m, a2m = masked(a1, a2, dtype)
    starts = segment_starts(a1m, a2m)
    at, inside, (gs, s1, s2) = _gathered(starts, n, [g, a1m, a2m], dtype)
    lam = np.empty(n, dtype=dtype)
    lam[at[inside]] = adjoint_state(s1, s2, gs, True, dtype)[inside]
    return (lam, *coefficient_gradients(lam, y, True, dtype))
