"""Serial loop of ONE CHUNK of a cascade of time-varying direct-form-I sections with a state that enters and one that leaves
(rf_var2_plan_execute_cascade_frames_stream), the yardstick of tests/test_stream_host.py, in the arithmetic of `dtype`.  `sections`
is K tuples (b0, b1, b2, a1, a2) of per-sample coefficients shaped like x, (N,) or (L, N) -- the chunk's own, no slot masked: the
six slots the calls without a state never read multiply the history here.

    state   (..., K + 1, 2): pair 0 the history of the input, pair k + 1 that of section k's result, each (the sample one place
            before the chunk, the sample two places before it) in the direction of the recurrence; None: zeros
    causal  v[n] = b0[n] s[n] + b1[n] s[n-1] + b2[n] s[n-2]        y[n] = v[n] - a1[n] y[n-1] - a2[n] y[n-2]
            with s[-1], s[-2] and y[-1], y[-2] from the state; the anticausal chunk is the causal one on every signal reversed

Chunks chained through their states are the unchunked cascade (tests/cascade_loops.py on the whole signal): test_stream_host.py
pins that to 1e-12 of the peak in f64."""
import numpy as np


def forward(x, sections, state=None, causal=True, dtype=np.float64):
    """([y_0, ..., y_{K-1}], the state that leaves) of one chunk"""
    x = np.asarray(x, dtype=dtype)
    K = len(sections)
    if not causal:
        ys, leaving = forward(x[..., ::-1], [tuple(np.asarray(c)[..., ::-1] for c in s) for s in sections], state, True, dtype)
        return [y[..., ::-1] for y in ys], leaving
    n = x.shape[-1]
    entering = np.zeros(x.shape[:-1] + (K + 1, 2), dtype) if state is None else np.asarray(state, dtype=dtype)
    leaving = np.empty_like(entering)
    leaving[..., 0, 0], leaving[..., 0, 1] = x[..., n - 1], x[..., n - 2]
    ys, src = [], x
    for k, s in enumerate(sections):
        b0, b1, b2, a1, a2 = (np.asarray(c, dtype=dtype) for c in s)
        s1, s2 = entering[..., k, 0].copy(), entering[..., k, 1].copy()
        y1, y2 = entering[..., k + 1, 0].copy(), entering[..., k + 1, 1].copy()
        y = np.empty_like(x)
        for i in range(n):
            v = b0[..., i] * src[..., i] + b1[..., i] * s1 + b2[..., i] * s2
            r = v - a1[..., i] * y1 - a2[..., i] * y2
            y[..., i] = r
            s2, s1 = s1, src[..., i]
            y2, y1 = y1, r
        leaving[..., k + 1, 0], leaving[..., k + 1, 1] = y[..., n - 1], y[..., n - 2]
        ys.append(y)
        src = y
    return ys, leaving


def adjoint(x, sections, ys, g, state=None, grad_state_out=None, causal=True, dtype=np.float64):
    """(grad_x, [(grad_b0, grad_b1, grad_b2, grad_a1, grad_a2) of section k, per sample], grad_state_in) of one chunk: the
    reverse of `forward` for the loss sum(g * y_{K-1}) + sum(grad_state_out * the state that leaves); ys: forward's results"""
    x = np.asarray(x, dtype=dtype)
    K = len(sections)
    if not causal:
        rev = lambda a: np.asarray(a)[..., ::-1]      # noqa: E731
        gx, grads, gsi = adjoint(rev(x), [tuple(rev(c) for c in s) for s in sections], [rev(y) for y in ys], rev(g), state, grad_state_out, True, dtype)
        return gx[..., ::-1], [tuple(p[..., ::-1] for p in s) for s in grads], gsi
    n = x.shape[-1]
    entering = np.zeros(x.shape[:-1] + (K + 1, 2), dtype) if state is None else np.asarray(state, dtype=dtype)
    leaving = np.zeros_like(entering) if grad_state_out is None else np.asarray(grad_state_out, dtype=dtype)
    gsi = np.zeros_like(entering)
    grads = [None] * K
    gy = np.array(g, dtype=dtype)
    for k in range(K - 1, -1, -1):
        b0, b1, b2, a1, a2 = (np.asarray(c, dtype=dtype) for c in sections[k])
        src, y = (x if k == 0 else np.asarray(ys[k - 1], dtype=dtype)), np.asarray(ys[k], dtype=dtype)
        gy[..., n - 1] += leaving[..., k + 1, 0]
        gy[..., n - 2] += leaving[..., k + 1, 1]
        lam = np.zeros(x.shape[:-1] + (n + 2,), dtype)
        for i in range(n - 1, -1, -1):
            r = gy[..., i]
            if i + 1 < n:
                r = r - a1[..., i + 1] * lam[..., i + 1]
            if i + 2 < n:
                r = r - a2[..., i + 2] * lam[..., i + 2]
            lam[..., i] = r
        lam = lam[..., :n]
        before = lambda s, h, d: np.concatenate([h[..., None, 1], h[..., None, 0], s], axis=-1)[..., 2 - d:n + 2 - d]      # noqa: E731
        hx, hy = entering[..., k, :], entering[..., k + 1, :]
        grads[k] = (lam * src, lam * before(src, hx, 1), lam * before(src, hx, 2), -lam * before(y, hy, 1), -lam * before(y, hy, 2))
        gsi[..., k + 1, 0] += -a1[..., 0] * lam[..., 0] - a2[..., 1] * lam[..., 1]
        gsi[..., k + 1, 1] += -a2[..., 0] * lam[..., 0]
        gsi[..., k, 0] += b1[..., 0] * lam[..., 0] + b2[..., 1] * lam[..., 1]
        gsi[..., k, 1] += b2[..., 0] * lam[..., 0]
        gs = b0 * lam
        gs[..., :n - 1] += (b1 * lam)[..., 1:]
        gs[..., :n - 2] += (b2 * lam)[..., 2:]
        gy = gs
    gy[..., n - 1] += leaving[..., 0, 0]
    gy[..., n - 2] += leaving[..., 0, 1]
    return gy, grads, gsi
