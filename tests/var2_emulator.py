"""The tiled algebra of kernels_var2_signal.hip replayed in numpy f32 on ONE line: tile tails (E and the 2 x 2 matrix P from three
recurrences in one sweep), the Kogge-Stone scan of (E, P) across the 64 lanes of a group, the sweep over groups 1024 at a time (wave
scans, the waves' totals folded in order) and the rerun from the entering state.  Every product-and-add the kernels write as an fma
is one here: the product and the sum in f64, rounded once to f32 (the product of two f32 is exact in f64).

An anticausal scan runs the same steps on the padded line reversed, as the kernels do: the samples a partial group lacks come
FIRST in the order of the recurrence.  adjoint=True: the coefficients shifted by one (a1) and two (a2) samples, the masks those of
the scan's own direction."""
import numpy as np

T = 64                 # samples of a tile
GROUP = 64             # tiles of a group
SWEEP = 1024           # groups of a sweep
F = np.float32


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def step2(c1, c2, x, y1, y2):
    return fma(-c1, y1, fma(-c2, y2, x))


def identity(shape):
    z, o = np.zeros(shape, F), np.ones(shape, F)
    return (z, z.copy(), o, z.copy(), z.copy(), o.copy())      # e0, e1, p00, p01, p10, p11


def compose(A, B):
    """sub-line A followed by B:  E = E_B + P_B E_A,  P = P_B P_A  (the order of operations of the kernels)"""
    ae0, ae1, a00, a01, a10, a11 = A
    be0, be1, b00, b01, b10, b11 = B
    return (fma(b00, ae0, fma(b01, ae1, be0)), fma(b10, ae0, fma(b11, ae1, be1)),
            fma(b00, a00, b01 * a10), fma(b00, a01, b01 * a11), fma(b10, a00, b11 * a10), fma(b10, a01, b11 * a11))


def apply_map(m, s0, s1):
    e0, e1, p00, p01, p10, p11 = m
    return fma(p00, s0, fma(p01, s1, e0)), fma(p10, s0, fma(p11, s1, e1))


def lane_scan(own, compose=compose):
    """inclusive Kogge-Stone scan along the last axis (64 lanes)"""
    whole = tuple(c.copy() for c in own)
    lanes = whole[0].shape[-1]
    k = 1
    while k < lanes:
        other = tuple(np.concatenate([c[..., :k], c[..., :-k]], axis=-1) for c in whole)      # (the first k: not taken)
        nxt = compose(other, whole)
        for c, v in zip(whole, nxt):
            c[..., k:] = v[..., k:]
        k *= 2
    return whole


def exclusive(whole):
    ident = identity(whole[0].shape[:-1] + (1,))
    return tuple(np.concatenate([i, c[..., :-1]], axis=-1) for i, c in zip(ident, whole))


def scan_coefficients(a1, a2, causal, adjoint):
    """(c1, c2) of the recurrence the kernels run, by position in the line: shifted where adjoint, masked by the direction"""
    n = a1.shape[0]
    c1 = np.array(a1, dtype=F)
    c2 = np.array(a2, dtype=F)
    at = np.arange(n)
    if adjoint and not causal:      # the adjoint of a causal scan runs anticausally and reads a1[n+1], a2[n+2]
        c1 = c1[np.minimum(at + 1, n - 1)]
        c2 = c2[np.minimum(at + 2, n - 1)]
    elif adjoint:
        c1 = c1[np.maximum(at - 1, 0)]
        c2 = c2[np.maximum(at - 2, 0)]
    if causal:
        c1[at < 1] = 0
        c2[at < 2] = 0
    else:
        c1[at >= n - 1] = 0
        c2[at >= n - 2] = 0
    return c1, c2


def tiled_scan(x, a1, a2, causal=True, adjoint=False, parts=None, mutate_aggregate=None, carry_compose=compose):
    """the three launches on one line (N,), N a multiple of 4.  `causal`: the direction of THIS recurrence.  parts: a dict that
    receives the intermediate values (tests).  mutate_aggregate, carry_compose: what tests/test_var2_carry_seen_host.py hands the
    carry stage in place of the groups' aggregates and of `compose` in its lane scan; left alone, no bit changes"""
    n = x.shape[0]
    c1, c2 = scan_coefficients(a1, a2, causal, adjoint)
    groups = -(-n // (T * GROUP))
    full = groups * T * GROUP

    def laid_out(v):
        p = np.zeros(full, F)
        p[:n] = v
        return (p if causal else p[::-1]).reshape(groups, GROUP, T)
    X, C1, C2 = laid_out(np.asarray(x, dtype=F)), laid_out(c1), laid_out(c2)
    # var2_tails_1d: three recurrences per tile
    shape = (groups, GROUP)
    y1, y2 = np.zeros(shape, F), np.zeros(shape, F)
    u1, u2 = np.ones(shape, F), np.zeros(shape, F)
    w1, w2 = np.zeros(shape, F), np.ones(shape, F)
    zero = np.zeros(shape, F)
    for i in range(T):
        y = step2(C1[..., i], C2[..., i], X[..., i], y1, y2)
        u = step2(C1[..., i], C2[..., i], zero, u1, u2)
        w = step2(C1[..., i], C2[..., i], zero, w1, w2)
        y2, y1, u2, u1, w2, w1 = y1, y, u1, u, w1, w
    own = (y1, y2, u1, w1, u2, w2)                    # e0, e1, p00, p01, p10, p11
    whole = lane_scan(own)
    maps = exclusive(whole)
    aggregate = tuple(c[:, -1] for c in whole)
    if mutate_aggregate is not None:
        aggregate = tuple(np.asarray(c, dtype=F) for c in mutate_aggregate(aggregate))
    # var2_carry_1d: sweeps of up to 1024 groups
    span = min(SWEEP, -(-groups // 64) * 64)
    carry0, carry1 = np.zeros(groups, F), np.zeros(groups, F)
    run0, run1 = F(0), F(0)
    for base in range(0, groups, span):
        take = min(span, groups - base)
        m = identity((span,))
        for c, a in zip(m, aggregate):
            c[:take] = a[base:base + take]
        m = tuple(c.reshape(span // 64, 64) for c in m)
        scanned = lane_scan(m, carry_compose)
        totals = tuple(c[:, -1] for c in scanned)
        enter0, enter1 = np.zeros(span // 64, F), np.zeros(span // 64, F)
        nxt0, nxt1 = np.array(run0, F), np.array(run1, F)
        for wv in range(span // 64):
            enter0[wv], enter1[wv] = nxt0, nxt1
            nxt0, nxt1 = apply_map(tuple(c[wv] for c in totals), nxt0, nxt1)
        ex = exclusive(scanned)
        g0, g1 = apply_map(ex, enter0[:, None], enter1[:, None])
        carry0[base:base + take] = g0.reshape(-1)[:take]
        carry1[base:base + take] = g1.reshape(-1)[:take]
        run0, run1 = nxt0, nxt1
    # var2_pass2_1d: the entering state of every tile, then the recurrence again
    y1, y2 = apply_map(maps, carry0[:, None], carry1[:, None])
    if parts is not None:
        parts.update(own=own, maps=maps, aggregate=aggregate, carry=(carry0, carry1), enter=(y1.copy(), y2.copy()))
    out = np.empty_like(X)
    for i in range(T):
        y = step2(C1[..., i], C2[..., i], X[..., i], y1, y2)
        out[..., i] = y
        y2, y1 = y1, y
    out = out.reshape(-1)
    return (out if causal else out[::-1])[:n].copy()


def tiled_forward(x, a1, a2, causal=True):
    return tiled_scan(x, a1, a2, causal, False)


def tiled_adjoint(a1, a2, y, g, causal=True):
    """(grad_x, grad_a1, grad_a2) as the backward's four launches form them; `causal`: the FORWARD's direction"""
    lam = tiled_scan(g, a1, a2, not causal, True)
    n = lam.shape[0]
    y = np.asarray(y, dtype=F)
    g1, g2 = np.zeros(n, F), np.zeros(n, F)
    if causal:
        g1[1:] = -lam[1:] * y[:-1]
        g2[2:] = -lam[2:] * y[:-2]
    else:
        g1[:-1] = -lam[:-1] * y[1:]
        g2[:-2] = -lam[:-2] * y[2:]
    return lam, g1, g2
