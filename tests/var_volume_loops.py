"""The varying scans and their adjoints on (D, H, W) volumes as serial numpy loops in a chosen float type (a plain module: no
fixtures): the loops of tests/var_grad_loops.py applied along any axis -- the scanned axis is moved last and the volume reshaped
to lines, so a line's arithmetic is that of a row of a 2-D image.  dim 0 = x (numpy axis 2), 1 = y (axis 1), 2 = z (axis 0).
The yardstick of tests/test_var_volume_host.py, tests/test_gpu_var_volume.py and tests/test_gpu_smooth_volume.py.

The power form is smooth_grad_loops' : w = exp2(d * log2 a), dL/dd = (w ln a) dL/dw, with the library's f32 constants in f32.
distances: the three exponent volumes of rf_var_distances_volume."""
import numpy as np

import smooth_grad_loops as power_loops
import var_grad_loops as loops

AXIS = {0: 2, 1: 1, 2: 0}


def to_lines(a, dim):
    """(lines, N) with the axis of `dim` last"""
    moved = np.moveaxis(np.asarray(a), AXIS[dim], -1)
    return np.ascontiguousarray(moved).reshape(-1, moved.shape[-1])


def from_lines(lines, shape, dim):
    """the (D, H, W) volume of `shape` whose lines along `dim` are the rows of `lines`"""
    moved_shape = tuple(np.moveaxis(np.empty(shape, dtype=np.uint8), AXIS[dim], -1).shape)
    return np.ascontiguousarray(np.moveaxis(lines.reshape(moved_shape), -1, AXIS[dim]))


def forward(volumes, weights, scans, dtype):
    """every scan's input and output: saved[q][pl] enters scan q, saved[len(scans)] is the result"""
    saved = [[np.asarray(v, dtype=dtype) for v in volumes]]
    for dim, causal, k in scans:
        wt = loops.masked_weights(to_lines(weights[k], dim), dtype)
        saved.append([from_lines(loops.scan(to_lines(v, dim), wt, causal), v.shape, dim) for v in saved[-1]])
    return saved


def reference(volumes, weights, scans, dtype):
    return forward(volumes, weights, scans, dtype)[-1]


def backward(volumes, weights, scans, grad_outs, dtype):
    """(grad_ins, grad_weights); grad_weights[k] is None for a weight volume no scan reads.  Planes are summed in index order, the
    scans that read a volume in the order the adjoint meets them."""
    saved = forward(volumes, weights, scans, dtype)
    g = [np.asarray(p, dtype=dtype) for p in grad_outs]
    grad_w = [None] * len(weights)
    for q in range(len(scans) - 1, -1, -1):
        dim, causal, k = scans[q]
        wt = loops.masked_weights(to_lines(weights[k], dim), dtype)
        total = None
        for pl in range(len(g)):
            dx, dw = loops.scan_adjoint(to_lines(g[pl], dim), to_lines(saved[q][pl], dim), to_lines(saved[q + 1][pl], dim), wt, causal)
            g[pl] = from_lines(dx, g[pl].shape, dim)
            total = dw if total is None else total + dw
        total = from_lines(total, g[0].shape, dim)
        grad_w[k] = total if grad_w[k] is None else grad_w[k] + total
    return g, grad_w


def power_weights(exponents, bases, dtype):
    return [power_loops.power_weights(d, a, dtype) for d, a in zip(exponents, bases)]


def power_backward(volumes, exponents, bases, scans, grad_outs, dtype):
    """(grad_ins, grad_exponents) of a scan list in the power form (smooth_grad_loops.power_backward on volumes)"""
    ws = power_weights(exponents, bases, dtype)
    grad_in, grad_w = backward(volumes, ws, scans, grad_outs, dtype)
    grad_d = []
    for w, a, gw in zip(ws, bases, grad_w):
        if gw is None:
            grad_d.append(None)
            continue
        with np.errstate(invalid="ignore"):
            gd = (w * power_loops.constants(a, dtype)[1]) * gw
        grad_d.append(np.where(gw == 0, dtype(0), gd).astype(dtype))
    return grad_in, grad_d


def distances(guide, scale, spacing_z, dtype):
    """[d_x, d_y, d_z] of a (C, D, H, W) guide in `dtype`, channels summed in index order"""
    g = np.asarray(guide, dtype=dtype)
    s = dtype(scale)
    sums = [np.zeros(g.shape[1:], dtype=dtype) for _ in range(3)]
    for ch in range(g.shape[0]):
        sums[0][:, :, 1:] += np.abs(g[ch][:, :, 1:] - g[ch][:, :, :-1])
        sums[1][:, 1:, :] += np.abs(g[ch][:, 1:, :] - g[ch][:, :-1, :])
        sums[2][1:, :, :] += np.abs(g[ch][1:, :, :] - g[ch][:-1, :, :])
    dx, dy, dz = dtype(1) + s * sums[0], dtype(1) + s * sums[1], dtype(spacing_z) + s * sums[2]
    dx[:, :, 0] = 1
    dy[:, 0, :] = 1
    dz[0, :, :] = dtype(spacing_z)
    return [dx.astype(dtype), dy.astype(dtype), dz.astype(dtype)]
