"""The adjoints behind rf_var_plan_backward_power, rf_var_distances_backward and rf_smooth_plan_backward as serial numpy loops in a
chosen float type (a plain module: no fixtures), built on tests/var_grad_loops.py (the plane form's adjoint) and
tests/smooth_cases.py (the forward conventions): the yardstick of tests/test_smooth_grad_host.py and
tests/test_gpu_smooth_grad.py.

    power form   w = exp2(d * l),  l = log2(base);   dL/dd = (w * c) * dL/dw,  c = ln(base);  d itself is never a factor, and where
                 dL/dw is exactly 0 (element 0 along the scanned dimension, by the plane form's select) so is dL/dd
    distances    d_x[r][c] = 1 + scale * sum_ch |g[r][c] - g[r][c-1]|  (c >= 1; 1 at c = 0), d_y likewise along rows
      adjoint    gg[ch][r][c] = scale * (sx(r,c) gdx[r][c] - sx(r,c+1) gdx[r][c+1] + sy(r,c) gdy[r][c] - sy(r+1,c) gdy[r+1][c])
                 sx / sy: the sign of the difference to the left / above, 0 outside the plane and for a difference of 0
    the filter   K iterations of +x -x +y -y in the power form on (d_x, d_y) with the bases {a_k, a_k}; its adjoint takes the
                 iterations in reverse order, and the gradients of d_x, d_y are summed in that order (k = K-1 first: the order in
                 which the plan adds them)
In f32 the constants are what the library forms: l = (float)log2((double)a), c = (float)log((double)a), a an f32."""
import numpy as np

import smooth_cases as sc
import var_grad_loops as loops


def constants(base, dtype):
    """(l, c) = (log2 a, ln a) of the f32 base a, rounded to `dtype`"""
    a = np.float64(np.float32(base))
    return dtype(np.log2(a)), dtype(np.log(a))


def power_weights(d, base, dtype):
    """the weight plane of an exponent plane: smooth_cases' conventions (f32: one f32 product, then exp2)"""
    d = np.asarray(d)
    with np.errstate(invalid="ignore"):
        w = sc.weights_f64(d, base) if dtype == np.float64 else sc.weights_f32(d.astype(np.float32), base)
    return w.astype(dtype, copy=False)


def power_backward(planes, exponents, bases, scans, grad_outs, dtype):
    """(grad_ins, grad_exponents) of a scan list in the power form; grad_exponents[k] is None for a plane no scan reads"""
    ws = [power_weights(d, a, dtype) for d, a in zip(exponents, bases)]
    grad_in, grad_w = loops.backward(planes, ws, scans, grad_outs, dtype)
    grad_d = []
    for w, a, gw in zip(ws, bases, grad_w):
        if gw is None:
            grad_d.append(None)
            continue
        with np.errstate(invalid="ignore"):
            gd = (w * constants(a, dtype)[1]) * gw
        grad_d.append(np.where(gw == 0, dtype(0), gd).astype(dtype))
    return grad_in, grad_d


def distances(guide, scale, dtype):
    """[d_x, d_y] of a (C, H, W) guide in `dtype`, channels summed in index order"""
    g = np.asarray(guide, dtype=dtype)
    s = dtype(scale)
    sx = np.zeros(g.shape[1:], dtype=dtype)
    sy = np.zeros(g.shape[1:], dtype=dtype)
    for ch in range(g.shape[0]):
        sx[:, 1:] += np.abs(g[ch][:, 1:] - g[ch][:, :-1])
        sy[1:, :] += np.abs(g[ch][1:, :] - g[ch][:-1, :])
    dx, dy = dtype(1) + s * sx, dtype(1) + s * sy
    dx[:, 0] = 1
    dy[0, :] = 1
    return [dx.astype(dtype), dy.astype(dtype)]


def distances_backward(guide, scale, gdx, gdy, dtype):
    """the (C, H, W) gradient of the guide from those of d_x and d_y, the four terms in the order the header gives"""
    g = np.asarray(guide, dtype=dtype)
    gdx, gdy = np.asarray(gdx, dtype=dtype), np.asarray(gdy, dtype=dtype)
    C, H, W = g.shape
    out = np.empty_like(g)
    for ch in range(C):
        left, up = np.zeros((H, W + 1), dtype=dtype), np.zeros((H + 1, W), dtype=dtype)      # sx(r, c) gdx[r][c], c = 0 .. W
        left[:, 1:W] = np.sign(g[ch][:, 1:] - g[ch][:, :-1]) * gdx[:, 1:]
        up[1:H, :] = np.sign(g[ch][1:, :] - g[ch][:-1, :]) * gdy[1:, :]
        out[ch] = dtype(scale) * (((left[:, :W] - left[:, 1:]) + up[:H, :]) - up[1:, :])
    return out


def smooth_forward(image, ds, bases, dtype):
    """inputs[k] = the planes that enter iteration k; inputs[K] = the result"""
    inputs = [[np.asarray(p, dtype=dtype) for p in image]]
    for a in bases:
        ws = [power_weights(d, a, dtype) for d in ds]
        inputs.append(loops.forward(inputs[-1], ws, sc.SCANS, dtype)[-1])
    return inputs


def smooth_backward(image, guide, bases, scale, grad_out, dtype, edges, order="plan"):
    """(grad_image (C, H, W), grad_guide or None, [gd_x, gd_y] or None) of the whole filter.  guide=None: the image guides itself,
    and with edges the guide's gradient is added to the image's.  order: "plan" sums the iterations' contributions to gd_x, gd_y
    with k = K-1 first, "forward" with k = 0 first (the same sum in exact arithmetic)."""
    self_guided = guide is None
    gd_src = image if self_guided else guide
    ds = distances(gd_src, scale, dtype)
    K = len(bases)
    inputs = smooth_forward(image, ds, bases, dtype)
    g = [np.asarray(p, dtype=dtype) for p in grad_out]
    per_k = [None] * K
    for k in range(K - 1, -1, -1):
        g, per_k[k] = power_backward(inputs[k], ds, [bases[k], bases[k]], sc.SCANS, g, dtype)
    grad_image = np.stack(g)
    if not edges:
        return grad_image, None, None
    ks = range(K - 1, -1, -1) if order == "plan" else range(K)
    gd = None
    for k in ks:
        gd = per_k[k] if gd is None else [a + b for a, b in zip(gd, per_k[k])]
    gg = distances_backward(gd_src, scale, gd[0], gd[1], dtype)
    if self_guided:
        return grad_image + gg, None, gd
    return grad_image, gg, gd


def torch_filter(image, guide, bases, scale, dtype):
    """the same filter in plain torch on CPU tensors (C, H, W) in `dtype`: Python loops over the scanned dimension, vectorised over
    the lines, differentiable by torch's autograd.  guide=None: the image guides itself.  Weights are exp2(d * log2 a_k), a_k f32."""
    import torch

    def scan(v, w, causal):      # along the last dimension of (C, L, N); w: (L, N), element 0 never read
        n = v.shape[-1]
        cols, acc = [None] * n, torch.zeros_like(v[..., 0])
        for i in (range(n) if causal else range(n - 1, -1, -1)):
            j = i if causal else i + 1
            acc = v[..., i] if j == 0 or j == n else (1 - w[:, j]) * v[..., i] + w[:, j] * acc
            cols[i] = acc
        return torch.stack(cols, dim=-1)
    v = image.to(dtype)
    gd = v if guide is None else guide.to(dtype)
    one_col, one_row = torch.ones_like(gd[0, :, :1]), torch.ones_like(gd[0, :1, :])
    dx = torch.cat([one_col, 1 + scale * (gd[:, :, 1:] - gd[:, :, :-1]).abs().sum(0)], dim=1)
    dy = torch.cat([one_row, 1 + scale * (gd[:, 1:, :] - gd[:, :-1, :]).abs().sum(0)], dim=0)
    for a in bases:
        l = float(np.log2(np.float64(np.float32(a))))
        wx, wy = torch.exp2(dx * l), torch.exp2(dy * l)
        v = scan(scan(v, wx, True), wx, False)
        v = scan(scan(v.transpose(1, 2), wy.t(), True), wy.t(), False).transpose(1, 2)
    return v
