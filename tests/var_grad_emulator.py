"""The tiled algebra of the adjoint stages and of var_grad (kernels_var.hip, rf_var_plan_backward) in numpy f32 (a plain module: no
fixtures).  Conventions of tests/var_scan_emulator.py: lines are the rows of a (lines, N) array.

An adjoint stage is a unit-gain scan  s[i] = g[i] + w s[neighbour]  in the direction opposite to its forward scan:
    tails    per tile, zero entry: E = the local scan's last value;  P = w~[t0] ... w~[t1-1]  (a causal recurrence: P1)  or
             w~[t0+1] ... w~[t1]  (an anticausal one: P2)
    carry    c_0 = 0, c_{t+1} = E_t + P_t c_t   /   d_{M-1} = 0, d_{t-1} = E_t + P_t d_t          (var_carry, unchanged)
    final    the recurrence again from the carry; stores (1 - w~) * s, and s itself for var_grad
var_grad sums  s (y' - x')  over the planes in index order, in f32, and stores it or adds it to what the gradient plane holds."""
import numpy as np

import var_scan_emulator as emu

f = np.float32


def tiled_adjoint_state(g, wt, causal, tile=64):
    """the adjoint state of a scan (causal: of the CAUSAL forward scan, so the recurrence here runs anticausally) as the three
    kernels of a stage compute it; g: (lines, N) f32, wt: emu.masked_weights in f32"""
    lines, n = g.shape
    m = (n + tile - 1) // tile
    zero = np.zeros(lines, dtype=f)

    def local(t, entry):
        t0, t1 = t * tile, min((t + 1) * tile, n)
        s = np.empty((lines, t1 - t0), dtype=f)
        acc = entry
        for i in (range(t1 - 1, t0 - 1, -1) if causal else range(t0, t1)):
            acc = g[:, i] + (wt[:, i + 1] if causal else wt[:, i]) * acc
            s[:, i - t0] = acc
        return s

    E = np.zeros((m, lines), dtype=f)
    P = np.zeros((m, lines), dtype=f)
    for t in range(m):
        t0, t1 = t * tile, min((t + 1) * tile, n)
        s = local(t, zero)
        E[t] = s[:, 0] if causal else s[:, -1]
        P[t] = np.multiply.reduce(wt[:, t0 + 1:t1 + 1] if causal else wt[:, t0:t1], axis=1, dtype=f)
    carry = np.zeros((m, lines), dtype=f)
    if causal:
        for t in range(m - 1, 0, -1):
            carry[t - 1] = E[t] + P[t] * carry[t]
    else:
        for t in range(m - 1):
            carry[t + 1] = E[t] + P[t] * carry[t]
    out = np.empty_like(g)
    for t in range(m):
        out[:, t * tile:min((t + 1) * tile, n)] = local(t, carry[t])
    return out


def var_grad(states, xs, ys, causal, dim):
    """one var_grad launch: (H, W) planes, summed in index order in f32; element 0 along `dim` is 0"""
    total = None
    for s, x, y in zip(states, xs, ys):
        if dim == 1:
            s, x, y = s.T, x.T, y.T
        term = np.zeros(s.shape, dtype=f)
        if causal:
            term[:, 1:] = s[:, 1:] * (y[:, :-1] - x[:, 1:])
        else:
            term[:, 1:] = s[:, :-1] * (y[:, 1:] - x[:, :-1])
        total = term if total is None else total + term
    total[:, 0] = 0
    return np.ascontiguousarray(total.T) if dim == 1 else total


def _lines(a, dim):
    return a if dim == 0 else np.ascontiguousarray(a.T)


def backward(planes, weights, scans, grad_outs, tile=64):
    """rf_var_plan_backward with every weight gradient: the forward rerun scan by scan (single-scan stages of
    var_scan_emulator.tiled_stage), then per scan in reverse order the adjoint stage and var_grad.  Returns
    (grad_ins, grad_weights); None for a weight plane no scan reads."""
    saved = [[np.asarray(p, dtype=f) for p in planes]]
    for dim, causal, k in scans:
        w = _lines(np.asarray(weights[k]), dim)
        saved.append([_lines(emu.tiled_stage(_lines(v, dim), w, emu.CAUSAL if causal else emu.ANTICAUSAL, tile), dim) for v in saved[-1]])
    g = [np.asarray(p, dtype=f) for p in grad_outs]
    grad_w = [None] * len(weights)
    for q in range(len(scans) - 1, -1, -1):
        dim, causal, k = scans[q]
        wt = emu.masked_weights(_lines(np.asarray(weights[k]), dim), f)
        n = wt.shape[1] - 1
        states = []
        for pl in range(len(g)):
            s = tiled_adjoint_state(_lines(g[pl], dim), wt, causal, tile)
            g[pl] = _lines((f(1) - (wt[:, :n] if causal else wt[:, 1:])) * s, dim)
            states.append(_lines(s, dim))
        total = var_grad(states, saved[q], saved[q + 1], causal, dim)
        grad_w[k] = total if grad_w[k] is None else grad_w[k] + total
    return g, grad_w
