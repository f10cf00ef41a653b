"""The backward of a plan of constant-coefficient scans (rf_plan_backward, include/recfilter_amd.h) restated over the CPU oracle.

Every scan, forward and transposed, is oracle.apply_filter; what the oracle cannot say -- the border term of a clamped scan's
transpose and the coefficient sums -- is written out below with numpy slices, per line in scan order r = 0 .. n-1:

    mu       = the unit-gain zero-border scan of g = dL/dy in the opposite direction (same feedback, feed-forward 1)
    dL/du    = c0 mu;   clamped: dL/du[0] += t_0 mu[0] + gamma sum_{1<=r<k} t_r mu[r],  t_r = sum_{j>=r} a_j,  gamma = c0 + t_0
    dL/da_j  = sum_{r>j} mu[r] y[r-j-1];   clamped: + beta + mu[0] u[0] + y[0] sum_{1<=r<=j} mu[r]
    dL/dc0   = sum_r mu[r] u[r];           clamped: + beta,   beta = u[0] sum_{1<=r<k} t_r mu[r]

dtype=np.float64 is the truth; dtype=np.float32 is the yardstick: every scan and every plane in f32 as a serial f32
implementation would hold them, the coefficient sums accumulated in f64 (as the kernels do).  Coefficients are rounded to f32
first in both, as the oracle does.
"""
from __future__ import annotations

import numpy as np

import oracle

RF_MAX_ORDER = 32


def _f32(v):
    return float(np.float32(v))


def _lines(a, dim, causal):
    """view of `a` with the scanned axis last and in scan order"""
    v = np.moveaxis(a, a.ndim - 1 - dim, -1)
    return v if causal else v[..., ::-1]


def forward_scans(x, scans, clamped):
    """[x, y_0, y_1, ...]: the filter scan by scan, in x's type"""
    ys = [np.ascontiguousarray(x)]
    for s in scans:
        ys.append(oracle.apply_filter(ys[-1], [s], clamped))
    return ys


def forward(x, scans, clamped, prologue=None, epilogue=None):
    """out = pf F(ps x + pb) + pi (ps x + pb) + po in x's type"""
    dt = x.dtype.type
    xp = x if prologue is None else dt(prologue[0]) * x + dt(prologue[1])
    f = oracle.apply_filter(np.ascontiguousarray(xp), list(scans), clamped)
    if epilogue is None:
        return f
    return dt(epilogue[0]) * f + dt(epilogue[1]) * xp + dt(epilogue[2])


def scan_backward(u, y, g, scan, clamped):
    """(dL/du, row, abs_row) of one scan: row = [dL/dc0, dL/da_0 ..] in f64 and the sums of its terms' magnitudes"""
    dim, causal, coeff = scan
    c0, a = _f32(coeff[0]), [_f32(c) for c in coeff[1:]]
    k = len(a)
    mu = oracle.apply_filter(np.ascontiguousarray(g), [(dim, not causal, [1.0] + a)], False)
    gn = (g.dtype.type(c0) * mu).astype(g.dtype)
    M, U, Y, G = (_lines(v, dim, causal) for v in (mu, u, y, gn))
    M64, U64, Y64 = (v.astype(np.float64) for v in (M, U, Y))
    n = M.shape[-1]
    row, mag = np.zeros(1 + RF_MAX_ORDER), np.zeros(1 + RF_MAX_ORDER)
    row[0], mag[0] = np.sum(M64 * U64), np.sum(np.abs(M64 * U64))
    for j in range(k):
        if n > j + 1:
            terms = M64[..., j + 1:] * Y64[..., :n - j - 1]
            row[1 + j], mag[1 + j] = np.sum(terms), np.sum(np.abs(terms))
    if clamped:
        assert n > k, "the clamped formulas are for lines longer than the order"
        t = [sum(a[r:]) for r in range(k)]
        gamma = c0 + t[0]
        tail = sum((t[r] * M64[..., r] for r in range(1, k)), np.zeros(M.shape[:-1]))
        G[..., 0] += (t[0] * M64[..., 0] + gamma * tail).astype(g.dtype)
        beta = U64[..., 0] * tail
        row[0] += np.sum(beta)
        mag[0] += np.sum(np.abs(beta))
        for j in range(k):
            sm = sum((M64[..., r] for r in range(1, j + 1)), np.zeros(M.shape[:-1]))
            terms = (beta, M64[..., 0] * U64[..., 0], Y64[..., 0] * sm)
            row[1 + j] += sum(np.sum(v) for v in terms)
            mag[1 + j] += sum(np.sum(np.abs(v)) for v in terms)
    return gn, row, mag


def backward(x, scans, clamped, g, dtype=np.float64, prologue=None, epilogue=None):
    """(grad_in, rows, mags): dL/dx of forward() for g = dL/d(out), and per scan the coefficient gradients (n_scans x 33, f64)
    with the sums of their terms' magnitudes (the filter reads x' = ps x + pb and its gradient enters as pf g)."""
    scans = list(scans)
    dt = np.dtype(dtype).type
    x, g = np.ascontiguousarray(x, dtype=dtype), np.ascontiguousarray(g, dtype=dtype)
    xp = x if prologue is None else dt(prologue[0]) * x + dt(prologue[1])
    ys = forward_scans(xp, scans, clamped)
    gf = g if epilogue is None else dt(epilogue[0]) * g
    rows, mags = np.zeros((len(scans), 1 + RF_MAX_ORDER)), np.zeros((len(scans), 1 + RF_MAX_ORDER))
    for s in range(len(scans) - 1, -1, -1):
        gf, rows[s], mags[s] = scan_backward(ys[s], ys[s + 1], gf, scans[s], clamped)
    if epilogue is not None:
        gf = gf + dt(epilogue[1]) * g
    if prologue is not None:
        gf = dt(prologue[0]) * gf
    return gf.astype(dtype), rows, mags
