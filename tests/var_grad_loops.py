"""The adjoint of the spatially varying first-order scans as serial numpy loops in a chosen float type (a plain module: no
fixtures): the yardstick of tests/test_var_grad_host.py and tests/test_gpu_var_grad.py.

Lines are the rows of a (lines, N) array; w[:, i] couples sample i-1 to sample i, w[:, 0] is never read.  With w~[0] = w~[N] = 0
and g = dL/dy:
    causal scan      y[i] = (1 - w~[i])   x[i] + w~[i]   y[i-1]
      adjoint        lam[i] = g[i] + w~[i+1] lam[i+1]        dL/dx[i] = (1 - w~[i])   lam[i]      dL/dw[i] = lam[i] (y[i-1] - x[i])
    anticausal scan  y[i] = (1 - w~[i+1]) x[i] + w~[i+1] y[i+1]
      adjoint        mu[i] = g[i] + w~[i] mu[i-1]            dL/dx[i] = (1 - w~[i+1]) mu[i]       dL/dw[i] = mu[i-1] (y[i] - x[i-1])
dL/dw[0] = 0.  A plan's adjoint runs its scans' adjoints in reverse order; the gradient of a weight plane is summed over the
image planes (in index order) and over the scans that read it (in the order the adjoint meets them)."""
import numpy as np


def masked_weights(w, dtype):
    """(lines, N + 1): w~[0] = w~[N] = 0 by assignment (element 0 of w is never read), w~[i] = w[i] otherwise"""
    lines, n = w.shape
    wt = np.zeros((lines, n + 1), dtype=dtype)
    wt[:, 1:n] = w[:, 1:n]
    return wt


def scan(x, wt, causal):
    """one forward scan along axis 1 in x's type; wt: masked_weights"""
    n = x.shape[1]
    one = x.dtype.type(1)
    y = np.empty_like(x)
    acc = np.zeros(x.shape[0], dtype=x.dtype)
    for i in (range(n) if causal else range(n - 1, -1, -1)):
        wi = wt[:, i] if causal else wt[:, i + 1]
        acc = (one - wi) * x[:, i] + wi * acc
        y[:, i] = acc
    return y


def adjoint_state(g, wt, causal):
    """lam (the adjoint of a causal scan: anticausal) or mu (of an anticausal scan: causal); unit input gain"""
    n = g.shape[1]
    s = np.empty_like(g)
    acc = np.zeros(g.shape[0], dtype=g.dtype)
    for i in (range(n - 1, -1, -1) if causal else range(n)):
        wi = wt[:, i + 1] if causal else wt[:, i]
        acc = g[:, i] + wi * acc
        s[:, i] = acc
    return s


def scan_adjoint(g, x, y, wt, causal):
    """(dL/dx, dL/dw) of one scan along axis 1 from g = dL/dy, the scan's input x and output y; everything in g's type"""
    n = g.shape[1]
    one = g.dtype.type(1)
    s = adjoint_state(g, wt, causal)
    dw = np.zeros_like(g)
    if causal:
        dx = (one - wt[:, :n]) * s
        dw[:, 1:] = s[:, 1:] * (y[:, :-1] - x[:, 1:])
    else:
        dx = (one - wt[:, 1:]) * s
        dw[:, 1:] = s[:, :-1] * (y[:, 1:] - x[:, :-1])
    return dx, dw


def _lines(a, dim):
    return a if dim == 0 else np.ascontiguousarray(a.T)


def forward(planes, weights, scans, dtype):
    """every scan's input and output: saved[q][pl] = the (H, W) plane that enters scan q; saved[len(scans)] = the result"""
    saved = [[np.asarray(p, dtype=dtype) for p in planes]]
    for dim, causal, k in scans:
        wt = masked_weights(_lines(np.asarray(weights[k]), dim), dtype)
        saved.append([_lines(scan(_lines(v, dim), wt, causal), dim) for v in saved[-1]])
    return saved


def backward(planes, weights, scans, grad_outs, dtype):
    """(grad_ins, grad_weights) of a scan list (dim, causal, weight index) on (H, W) planes; grad_weights has one entry per weight
    plane, None for a plane that no scan reads"""
    saved = forward(planes, weights, scans, dtype)
    g = [np.asarray(p, dtype=dtype) for p in grad_outs]
    grad_w = [None] * len(weights)
    for q in range(len(scans) - 1, -1, -1):
        dim, causal, k = scans[q]
        wt = masked_weights(_lines(np.asarray(weights[k]), dim), dtype)
        total = None
        for pl in range(len(g)):
            dx, dw = scan_adjoint(_lines(g[pl], dim), _lines(saved[q][pl], dim), _lines(saved[q + 1][pl], dim), wt, causal)
            g[pl] = _lines(dx, dim)
            total = dw if total is None else total + dw
        total = _lines(total, dim)
        grad_w[k] = total if grad_w[k] is None else grad_w[k] + total
    return g, grad_w
