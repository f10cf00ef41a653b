"""The adjoints behind rf_var_distances_volume_backward and rf_smooth_plan_backward on volumes as serial numpy loops in a chosen
float type (a plain module: no fixtures), built on tests/var_volume_loops.py (the volume scans, their power-form adjoint and the
three distance volumes): the yardstick of tests/test_smooth_volume_grad_host.py and tests/test_gpu_smooth_volume_grad.py.

    distances    d_x, d_y slice by slice as on images; d_z[z][r][c] = spacing_z + scale * sum_ch |g[z][r][c] - g[z-1][r][c]|
      adjoint    gg[ch][z][r][c] = scale * (((((L - R) + U) - Dn) + B) - A)
                 L = sx(z,r,c) gdx[z][r][c]   R = sx(z,r,c+1) gdx[z][r][c+1]   U = sy(z,r,c) gdy[z][r][c]   Dn = sy(z,r+1,c) gdy[z][r+1][c]
                 B = sz(z,r,c) gdz[z][r][c]   A = sz(z+1,r,c) gdz[z+1][r][c]
                 sx / sy / sz: the sign of the difference to the left / above / one slice before, 0 outside the volume and for a
                 difference of 0; spacing_z is an additive constant and does not enter
    the filter   K iterations of +x -x +y -y +z -z in the power form on (d_x, d_y, d_z) with the bases {a_k, a_k, a_k}; its adjoint
                 takes the iterations in reverse order, and the gradients of the distances are summed in that order (k = K-1
                 first: the order in which the plan adds them)"""
import numpy as np

import var_volume_loops as vloops

SCANS = [(0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1), (2, True, 2), (2, False, 2)]


def distances_backward(guide, scale, gdx, gdy, gdz, dtype):
    """the (C, D, H, W) gradient of the guide from those of d_x, d_y and d_z, the six terms in the order the header gives"""
    g = np.asarray(guide, dtype=dtype)
    gdx, gdy, gdz = (np.asarray(a, dtype=dtype) for a in (gdx, gdy, gdz))
    C, D, H, W = g.shape
    out = np.empty_like(g)
    for ch in range(C):
        # sx(z, r, c) gdx[z][r][c] for c = 0 .. W (0 at both ends), and the same along rows and slices
        left, up, before = np.zeros((D, H, W + 1), dtype=dtype), np.zeros((D, H + 1, W), dtype=dtype), np.zeros((D + 1, H, W), dtype=dtype)
        left[:, :, 1:W] = np.sign(g[ch][:, :, 1:] - g[ch][:, :, :-1]) * gdx[:, :, 1:]
        up[:, 1:H, :] = np.sign(g[ch][:, 1:, :] - g[ch][:, :-1, :]) * gdy[:, 1:, :]
        before[1:D, :, :] = np.sign(g[ch][1:, :, :] - g[ch][:-1, :, :]) * gdz[1:, :, :]
        out[ch] = dtype(scale) * (((((left[:, :, :W] - left[:, :, 1:]) + up[:, :H, :]) - up[:, 1:, :]) + before[:D]) - before[1:])
    return out


def smooth_forward(image, ds, bases, dtype):
    """inputs[k] = the volumes that enter iteration k; inputs[K] = the result"""
    inputs = [[np.asarray(p, dtype=dtype) for p in image]]
    for a in bases:
        inputs.append(vloops.reference(inputs[-1], vloops.power_weights(ds, [a, a, a], dtype), SCANS, dtype))
    return inputs


def smooth_backward(image, guide, bases, scale, spacing_z, grad_out, dtype, edges, order="plan"):
    """(grad_image (C, D, H, W), grad_guide or None, [gd_x, gd_y, gd_z] or None) of the whole filter.  guide=None: the volume
    guides itself, and with edges the guide's gradient is added to the volume's.  order: "plan" sums the iterations' contributions
    to the distance gradients with k = K-1 first, "forward" with k = 0 first (the same sum in exact arithmetic)."""
    self_guided = guide is None
    gd_src = image if self_guided else guide
    ds = vloops.distances(gd_src, scale, spacing_z, dtype)
    K = len(bases)
    inputs = smooth_forward(image, ds, bases, dtype)
    g = [np.asarray(p, dtype=dtype) for p in grad_out]
    per_k = [None] * K
    for k in range(K - 1, -1, -1):
        g, per_k[k] = vloops.power_backward(inputs[k], ds, [bases[k]] * 3, SCANS, g, dtype)
    grad_image = np.stack(g)
    if not edges:
        return grad_image, None, None
    ks = range(K - 1, -1, -1) if order == "plan" else range(K)
    gd = None
    for k in ks:
        gd = per_k[k] if gd is None else [a + b for a, b in zip(gd, per_k[k])]
    gg = distances_backward(gd_src, scale, gd[0], gd[1], gd[2], dtype)
    if self_guided:
        return grad_image + gg, None, gd
    return grad_image, gg, gd


def torch_distances(gd, scale, spacing_z):
    """[d_x, d_y, d_z] of a (C, D, H, W) torch tensor, differentiable by autograd (|.|'s derivative at 0 is 0 there too)"""
    import torch
    dx = torch.cat([torch.ones_like(gd[0, :, :, :1]), 1 + scale * (gd[:, :, :, 1:] - gd[:, :, :, :-1]).abs().sum(0)], dim=2)
    dy = torch.cat([torch.ones_like(gd[0, :, :1, :]), 1 + scale * (gd[:, :, 1:, :] - gd[:, :, :-1, :]).abs().sum(0)], dim=1)
    dz = torch.cat([torch.full_like(gd[0, :1], spacing_z), spacing_z + scale * (gd[:, 1:] - gd[:, :-1]).abs().sum(0)], dim=0)
    return [dx, dy, dz]


def torch_filter(image, guide, bases, scale, spacing_z, dtype):
    """the same filter in plain torch on CPU tensors (C, D, H, W) in `dtype`: Python loops over the scanned axis, vectorised over
    the lines, differentiable by torch's autograd.  guide=None: the volume guides itself.  Weights are exp2(d * log2 a_k), a_k f32."""
    import torch

    def scan(v, w, causal):      # along the last axis of (C, ..., N); w: (..., N), element 0 never read
        n = v.shape[-1]
        cols, acc = [None] * n, torch.zeros_like(v[..., 0])
        for i in (range(n) if causal else range(n - 1, -1, -1)):
            j = i if causal else i + 1
            acc = v[..., i] if j == 0 or j == n else (1 - w[..., j]) * v[..., i] + w[..., j] * acc
            cols[i] = acc
        return torch.stack(cols, dim=-1)

    def along(v, w, axis):       # +d then -d along `axis` of (C, D, H, W); w is (D, H, W)
        vm, wm = v.movedim(axis, -1), w.movedim(axis - 1, -1)
        return scan(scan(vm, wm, True), wm, False).movedim(-1, axis)
    v = image.to(dtype)
    ds = torch_distances(v if guide is None else guide.to(dtype), scale, spacing_z)
    for a in bases:
        l = float(np.log2(np.float64(np.float32(a))))
        for d, axis in zip(ds, (3, 2, 1)):
            v = along(v, torch.exp2(d * l), axis)
    return v
