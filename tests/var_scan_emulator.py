"""The tiling algebra of the spatially varying first-order scans (kernels_var.hip) in numpy f32 (a plain module: no fixtures).

Lines are the rows of a (lines, N) array; w[:, i] couples sample i-1 to sample i, w[:, 0] is never read.  With w~[0] = w~[N] = 0:
    causal      y[i] = (1 - w~[i])   x[i] + w~[i]   y[i-1]
    anticausal  y[i] = (1 - w~[i+1]) x[i] + w~[i+1] y[i+1]
`serial` is that recurrence in any float type; `tiled_stage` is what the three kernels of a stage compute, tile by tile:
tails (E1, P1, E2, G, P2) with zero entry, the carry recurrence over the tiles, and the final pass, which RERUNS the recurrences
from the completed carries.  G = v_p[t0], the anticausal scan of the prefix products, either as that scan (g_form="scan") or
written out as the sum the kernel forms, sum_i qq[i] (1 - w~[i+1]) p[i] with qq[i] = w~[t0+1] ... w~[i] (g_form="sum")."""
import numpy as np

CAUSAL, ANTICAUSAL, PAIR = 0, 1, 2


def masked_weights(w, dtype):
    """(lines, N + 1): w~[0] = w~[N] = 0 by assignment (element 0 of w is never read), w~[i] = w[i] otherwise"""
    lines, n = w.shape
    wt = np.zeros((lines, n + 1), dtype=dtype)
    wt[:, 1:n] = w[:, 1:n]
    return wt


def _causal(x, wt, entry, first):
    """x: (lines, T) samples of [first, first + T); returns the scan entered with `entry`"""
    y = np.empty_like(x)
    prev = entry
    one = x.dtype.type(1)
    for i in range(x.shape[1]):
        wi = wt[:, first + i]
        prev = (one - wi) * x[:, i] + wi * prev
        y[:, i] = prev
    return y


def _anticausal(x, wt, entry, first):
    y = np.empty_like(x)
    nxt = entry
    one = x.dtype.type(1)
    for i in range(x.shape[1] - 1, -1, -1):
        wi = wt[:, first + i + 1]
        nxt = (one - wi) * x[:, i] + wi * nxt
        y[:, i] = nxt
    return y


def serial(x, w, causal, dtype=np.float64):
    """one scan along axis 1, untiled, in `dtype`"""
    x = np.asarray(x, dtype=dtype)
    wt = masked_weights(w, dtype)
    zero = np.zeros(x.shape[0], dtype=dtype)
    return _causal(x, wt, zero, 0) if causal else _anticausal(x, wt, zero, 0)


def tiled_stage(x, w, mode, tile=64, g_form="sum"):
    """one stage (CAUSAL, ANTICAUSAL or PAIR = causal then anticausal) along axis 1 in f32, as the kernels tile it"""
    f = np.float32
    x = np.asarray(x, dtype=f)
    wt = masked_weights(w, f)
    lines, n = x.shape
    m = (n + tile - 1) // tile
    zero = np.zeros(lines, dtype=f)
    E1, P1, E2, G, P2 = (np.zeros((m, lines), dtype=f) for _ in range(5))
    for t in range(m):
        t0, t1 = t * tile, min((t + 1) * tile, n)
        xt = x[:, t0:t1]
        u = xt
        if mode != ANTICAUSAL:
            u = _causal(xt, wt, zero, t0)
            E1[t] = u[:, -1]
            P1[t] = np.multiply.reduce(wt[:, t0:t1], axis=1, dtype=f)
        if mode != CAUSAL:
            E2[t] = _anticausal(u, wt, zero, t0)[:, 0]
            P2[t] = np.multiply.reduce(wt[:, t0 + 1:t1 + 1], axis=1, dtype=f)
        if mode == PAIR:
            p = np.multiply.accumulate(wt[:, t0:t1], axis=1, dtype=f)
            if g_form == "scan":
                G[t] = _anticausal(p, wt, zero, t0)[:, 0]
            else:
                qq = np.ones(lines, dtype=f)
                g = np.zeros(lines, dtype=f)
                for i in range(t1 - t0):
                    if i > 0:
                        qq = qq * wt[:, t0 + i]
                    g = g + (qq * (f(1) - wt[:, t0 + i + 1])) * p[:, i]
                G[t] = g
    c = np.zeros((m, lines), dtype=f)
    d = np.zeros((m, lines), dtype=f)
    if mode != ANTICAUSAL:
        for t in range(m - 1):
            c[t + 1] = E1[t] + P1[t] * c[t]
    if mode != CAUSAL:
        for t in range(m - 1, 0, -1):
            d[t - 1] = E2[t] + P2[t] * d[t]
            if mode == PAIR:
                d[t - 1] = d[t - 1] + G[t] * c[t]
    y = np.empty_like(x)
    for t in range(m):
        t0, t1 = t * tile, min((t + 1) * tile, n)
        v = x[:, t0:t1]
        if mode != ANTICAUSAL:
            v = _causal(v, wt, c[t], t0)
        if mode != CAUSAL:
            v = _anticausal(v, wt, d[t], t0)
        y[:, t0:t1] = v
    return y


def apply_scans(planes, scans, weights, dtype=np.float64):
    """A plan's scan list (dim, causal, weight index) on (H, W) planes, untiled, in `dtype`: the reference of a whole plan"""
    out = []
    for plane in planes:
        v = np.asarray(plane, dtype=dtype)
        for dim, causal, k in scans:
            if dim == 0:
                v = serial(v, weights[k], bool(causal), dtype)
            else:
                v = np.ascontiguousarray(serial(v.T, np.asarray(weights[k]).T, bool(causal), dtype).T)
        out.append(v)
    return out
