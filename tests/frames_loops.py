"""Yardsticks of the direct-form-I section on control-rate frames (rf_var2_plan_execute_biquad_frames / _backward_biquad_frames),
on tests/biquad_loops.py.  A coefficient is F = ceil(N / H) + 1 frames per line, frame j at sample j H; at n = j H + k, 0 <= k < H,

    c[n] = fma(k / H, c[j+1] - c[j], c[j])          (`expand`)

by absolute position whatever the section's direction.  `contract` is the transpose of `expand`: S0_j = sum_k (1 - k / H) g[j H + k],
S1_j = sum_k (k / H) g[j H + k], out[j] = S0_j + S1_{j-1}.  `forward` and `adjoint` are biquad_loops' on the expansion, the five
per-sample coefficient gradients contracted.  Arrays are (N,) / (F,) or (L, N) / (L, F)."""
import numpy as np

import biquad_loops


def frames_count(n, hop):
    return -(-n // hop) + 1


def expand(frames, hop, n, dtype=np.float64):
    """np.float64: the formula in f64.  np.float32: the f32 value the kernels form -- the difference rounded to f32, then one
    fma: k / H and its product with an f32 are exact in f64, so the f64 sum rounded to f32 is the fma but for a double rounding
    that needs the f64 sum to fall on an f32 tie (it cannot where every c[n] is representable: test 1 of the GPU file)."""
    frames = np.asarray(frames, dtype=dtype)
    assert frames.shape[-1] == frames_count(n, hop), (frames.shape, n, hop)
    at = np.arange(n)
    j, w = at // hop, (at % hop) / float(hop)
    c0, c1 = frames[..., j], frames[..., j + 1]
    d = (c1 - c0).astype(dtype)
    return (w * d.astype(np.float64) + c0.astype(np.float64)).astype(dtype)


def contract(g, hop, count, dtype=np.float64):
    """the transpose of expand as a serial sum over every interval, in `dtype`"""
    g = np.asarray(g, dtype=dtype)
    n = g.shape[-1]
    assert count == frames_count(n, hop)
    padded = np.zeros(g.shape[:-1] + ((count - 1) * hop,), dtype=dtype)
    padded[..., :n] = g
    padded = padded.reshape(g.shape[:-1] + (count - 1, hop))
    w1 = (np.arange(hop) / float(hop)).astype(dtype)
    w0 = (1 - np.arange(hop) / float(hop)).astype(dtype)
    s0 = np.cumsum(padded * w0, axis=-1, dtype=dtype)[..., -1]      # (np.cumsum adds in order)
    s1 = np.cumsum(padded * w1, axis=-1, dtype=dtype)[..., -1]
    out = np.zeros(g.shape[:-1] + (count,), dtype=dtype)
    out[..., :-1] += s0
    out[..., 1:] += s1
    return out


def contraction_bound(g32, hop, count):
    """sum_k |w g32| per frame, in f64: what the f64 partial sums' rounding scales with"""
    return contract(np.abs(np.asarray(g32, dtype=np.float64)), hop, count)


def expand_all(frames5, hop, n, dtype=np.float64):
    return [expand(f, hop, n, dtype) for f in frames5]


def forward(x, frames5, hop, causal=True, dtype=np.float64):
    return biquad_loops.forward(x, *expand_all(frames5, hop, np.asarray(x).shape[-1], dtype), causal, dtype)


def adjoint(x, frames5, hop, y, g, causal=True, dtype=np.float64):
    """(grad_x, then the five frame gradients); the loops run in `dtype`, the contraction in f64 -- in f32 it would be a second
    yardstick of its own, and the kernels contract in f64"""
    count = np.asarray(frames5[0]).shape[-1]
    gx, *per_sample = biquad_loops.adjoint(x, *expand_all(frames5, hop, np.asarray(x).shape[-1], dtype), y, g, causal, dtype)
    return (gx, *(contract(p, hop, count, np.float64) for p in per_sample))
