"""The gradient of the BASES of the power form (rf_var_plan_backward_power_bases) as serial numpy loops in a chosen float type (a
plain module: no fixtures), built on tests/var_volume_loops.py -- and through it on tests/smooth_grad_loops.py and
tests/var_grad_loops.py: the yardstick of tests/test_sigma_grad_host.py and tests/test_gpu_sigma_grad.py.

    w[i] = exp2(d[i] * log2 base_k);  with s[i] = sum over the image planes of dL/dw[i] for ONE scan (planes in index order),
    dL/dbase_k = (1 / base_k) * sum over the scans that read plane k (in the order the adjoint meets them), over i, of t[i]
    t[i] = (w[i] == 0 ? 0 : d[i] * w[i] * s[i]);  element 0 along the scanned dimension contributes 0 by a select

Everything is a (D, H, W) volume here: an (H, W) image is the volume (1, H, W) with dims 0 and 1, a signal of N samples the volume
(1, 1, N) with dim 0 -- a line's arithmetic does not depend on its container.  In f32 every product and the running sum are f32,
the terms added serially in memory order; the normaliser sum |t| / base_k is always formed in f64."""
import numpy as np

import var_volume_loops as vloops
from var_volume_loops import loops


def as_volume(a):
    """a signal (N,), an image (H, W) or a volume (D, H, W) as a volume"""
    a = np.asarray(a)
    return a.reshape((1,) * (3 - a.ndim) + a.shape)


def serial_sum(t, dtype):
    """the terms added one after the other, in memory order, the running sum in `dtype`"""
    flat = np.ascontiguousarray(t, dtype=dtype).ravel()
    return dtype(0) if flat.size == 0 else np.cumsum(flat, dtype=dtype)[-1]


def base_terms(exponent, w, total, dim, dtype):
    """t of one scan along `dim` (as a volume): `total` is that scan's dL/dw summed over the image planes"""
    d = np.asarray(exponent, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.where(w == 0, dtype(0), (d * w) * total)
    first = [slice(None)] * 3
    first[vloops.AXIS[dim]] = 0
    t[tuple(first)] = 0                      # (a select: a NaN exponent at element 0 reaches nothing)
    return t.astype(dtype)


def power_bases_backward(planes, exponents, bases, scans, grad_outs, dtype, weights=None):
    """(grad_ins, grad_bases, normalisers) of a scan list in the power form.  grad_bases[k] = dL/dbases[k] as a `dtype` scalar, 0
    for a plane no scan reads; normalisers[k] = sum |t| / bases[k] in f64, the figure an error of grad_bases[k] is taken relative
    to.  planes / exponents / grad_outs: signals, images or volumes of one shape."""
    shape = np.asarray(planes[0]).shape
    vols = [as_volume(np.asarray(p, dtype=dtype)) for p in planes]
    ds = [as_volume(d) for d in exponents]
    ws = vloops.power_weights(ds, bases, dtype) if weights is None else [as_volume(w) for w in weights]      # (weights: formed by the caller)
    saved = vloops.forward(vols, ws, scans, dtype)
    g = [as_volume(np.asarray(p, dtype=dtype)) for p in grad_outs]
    sums = [dtype(0)] * len(bases)
    norms = [0.0] * len(bases)
    for q in range(len(scans) - 1, -1, -1):
        dim, causal, k = scans[q]
        wt = loops.masked_weights(vloops.to_lines(ws[k], dim), dtype)
        total = None
        for pl in range(len(g)):
            dx, dw = loops.scan_adjoint(vloops.to_lines(g[pl], dim), vloops.to_lines(saved[q][pl], dim), vloops.to_lines(saved[q + 1][pl], dim), wt, causal)
            g[pl] = vloops.from_lines(dx, g[pl].shape, dim)
            total = dw if total is None else total + dw
        t = base_terms(ds[k], ws[k], vloops.from_lines(total, g[0].shape, dim), dim, dtype)
        sums[k] = dtype(sums[k] + serial_sum(t, dtype))
        norms[k] += float(np.abs(t.astype(np.float64)).sum())
    a = [np.float64(np.float32(b)) if weights is None else np.float64(b) for b in bases]
    return ([p.reshape(shape) for p in g], [dtype(s / dtype(b)) for s, b in zip(sums, a)], [n / float(b) for n, b in zip(norms, a)])


# ---- the smoothing plan: dL/dsigma_s, dL/dsigma_r, dL/dspacing_z, dL/da_k ---------------------------------------------------------
IMAGE_SCANS = [(0, True, 0), (0, False, 0), (1, True, 1), (1, False, 1)]
VOLUME_SCANS = IMAGE_SCANS + [(2, True, 2), (2, False, 2)]


def smooth_bases(sigma_s, K, exact=False):
    """a_k = exp(-sqrt2 / (sigma_s c_k)), c_k = sqrt3 2^(K-1-k) / sqrt(4^K - 1): rounded to f32 as the plan rounds them, or exact"""
    a = [np.exp(-np.sqrt(2.0) / (sigma_s * np.sqrt(3.0) * 2.0 ** (K - 1 - k) / np.sqrt(4.0 ** K - 1.0))) for k in range(K)]
    return a if exact else [np.float64(np.float32(v)) for v in a]


def smooth_distances(guide, sigma_s, sigma_r, spacing_z, dtype, exact=False, byte_guide=False):
    """[d_x, d_y] of a (C, H, W) guide as volumes (1, H, W), or [d_x, d_y, d_z] of a (C, D, H, W) guide (spacing_z not None); the scale
    sigma_s / sigma_r (over 255 for a byte guide) rounded to f32 as the plan rounds it, or exact"""
    scale = sigma_s / sigma_r / (255.0 if byte_guide else 1.0)
    scale = scale if exact else float(np.float32(scale))
    g = np.asarray(guide, dtype=dtype)
    if spacing_z is None:
        g = g[:, None]
    ds = vloops.distances(g, scale, 1.0 if spacing_z is None else spacing_z, dtype)
    return ds[:2] if spacing_z is None else ds


def smooth_sigma_backward(image, guide, sigma_s, sigma_r, K, grad_out, dtype, spacing_z=None, exact=False, byte_guide=False):
    """(params, normalisers), 3 + K entries each: dL/dsigma_s, dL/dsigma_r, dL/dspacing_z, dL/da_0 .. dL/da_{K-1} of the smoothing
    filter on a (C, H, W) image or, with spacing_z, a (C, D, H, W) volume; guide=None: it guides itself.  With gd the exponent
    gradients summed over the iterations (k = K-1 first, as the plan adds them), A_k = dL/da_k summed over the dimensions and
    Q = sum gd (d - d0):  dL/dsigma_s = (sum_k A_k a_k (-ln a_k) + Q) / sigma_s,  dL/dsigma_r = -Q / sigma_r,  dL/dspacing_z = sum gd_z.
    exact: no rounding of the scale and the bases to f32 (what central differences in the sigmas see)."""
    volume = spacing_z is not None
    scans = VOLUME_SCANS if volume else IMAGE_SCANS
    n = len(scans) // 2
    bases = smooth_bases(sigma_s, K, exact)
    ds = smooth_distances(image if guide is None else guide, sigma_s, sigma_r, spacing_z, dtype, exact, byte_guide)
    vols = [np.asarray(p, dtype=dtype) if volume else np.asarray(p, dtype=dtype)[None] for p in image]
    consts = [(dtype(np.log2(a)), dtype(np.log(a))) for a in bases]

    def weights(k):
        with np.errstate(invalid="ignore"):
            return [np.exp2(d * consts[k][0]).astype(dtype) for d in ds]
    inputs = [vols]
    for k in range(K):
        inputs.append(vloops.reference(inputs[-1], weights(k), scans, dtype))
    g = [np.asarray(p, dtype=dtype) if volume else np.asarray(p, dtype=dtype)[None] for p in grad_out]
    gd, A, normA = None, [None] * K, [0.0] * K
    for k in range(K - 1, -1, -1):
        ws = weights(k)
        _, gw = vloops.backward(inputs[k], ws, scans, g, dtype)
        g, gb, nb = power_bases_backward(inputs[k], ds, [bases[k]] * n, scans, g, dtype, weights=ws)
        A[k] = dtype(sum(gb[1:], gb[0]))
        normA[k] = float(sum(nb))
        with np.errstate(invalid="ignore"):
            here = [np.where(w_ == 0, dtype(0), (w_ * consts[k][1]) * gw_).astype(dtype) for w_, gw_ in zip(ws, gw)]
        gd = here if gd is None else [p + q for p, q in zip(gd, here)]
    d0 = [dtype(1), dtype(1), dtype(1.0 if spacing_z is None else spacing_z)]
    Q, normQ = dtype(0), 0.0
    for q in range(n):
        with np.errstate(invalid="ignore"):
            t = np.where(gd[q] == 0, dtype(0), gd[q] * (ds[q] - d0[q])).astype(dtype)
        Q = dtype(Q + serial_sum(t, dtype))
        normQ += float(np.abs(t.astype(np.float64)).sum())
    ss, sr = dtype(sigma_s), dtype(sigma_r)
    from_bases = dtype(0)
    for k in range(K):
        from_bases = dtype(from_bases + A[k] * dtype(bases[k]) * dtype(-np.log(bases[k])))
    params = [dtype((from_bases + Q) / ss), dtype(-Q / sr), serial_sum(gd[2], dtype) if volume else dtype(0)] + A
    norms = [(sum(normA[k] * bases[k] * -np.log(bases[k]) for k in range(K)) + normQ) / sigma_s, normQ / sigma_r,
             float(np.abs(gd[2].astype(np.float64)).sum()) if volume else 0.0] + normA
    return params, norms


def figure(got, want, normaliser):
    """|got - want| / sum |terms|: the project's figure for a reduced scalar (tests/test_gpu_plan_grad.py).  No terms at all (a scan
    along a dimension of extent 1): the scalar is exactly 0, and anything else is infinitely far off."""
    if normaliser == 0:
        return 0.0 if float(got) == float(want) == 0.0 else float("inf")
    return abs(float(got) - float(want)) / normaliser


def bar(yard):
    """what a kernel's figure is held to, from the f32 loops' figure of the same entry"""
    return max(4.0 * yard, 1e-6)
