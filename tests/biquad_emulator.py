"""The direct-form-I section as the kernels form it, replayed in numpy f32 on ONE line, on top of tests/var2_emulator.py: the
feed-forward part of var2_biquad_tails_1d -- v = fma(b2~, x two before, fma(b1~, x one before, b0 * x)), the product b0 * x rounded
to f32, each fma rounded once -- in front of the emulator's three launches, and var2_biquad_grad_1d behind its adjoint scan:
grad_x = fma(b2~, lam two ahead, fma(b1~, lam one ahead, b0 * lam)), the coefficient gradients single f32 products.  Masked taps
are selected to 0; x and lam outside the line are 0."""
import numpy as np

import var2_emulator as emu
from biquad_loops import ahead, shifted

F = np.float32


def _taps(b0, b1, b2, causal):
    """(b0, b1~, b2~): the masks of the section's own direction, by a select"""
    b0, b1, b2 = (np.array(b, dtype=F) for b in (b0, b1, b2))
    if causal:
        b1[:1] = 0
        b2[:2] = 0
    else:
        b1[-1:] = 0
        b2[-2:] = 0
    return b0, b1, b2


def feed_forward(x, b0, b1, b2, causal=True):
    """v of var2_biquad_tails_1d, what the launch stores to `out`"""
    x = np.asarray(x, dtype=F)
    b0, b1, b2 = _taps(b0, b1, b2, causal)
    one, two = (shifted(x, 1), shifted(x, 2)) if causal else (ahead(x, 1), ahead(x, 2))
    return emu.fma(b2, two, emu.fma(b1, one, b0 * x))


def tiled_forward(x, b0, b1, b2, a1, a2, causal=True):
    return emu.tiled_scan(feed_forward(x, b0, b1, b2, causal), a1, a2, causal, False)


def tiled_adjoint(x, b0, b1, b2, a1, a2, y, g, causal=True):
    """(grad_x, grad_b0, grad_b1, grad_b2, grad_a1, grad_a2) as the backward's four launches form them; y: the forward's output"""
    lam = emu.tiled_scan(g, a1, a2, not causal, True)
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    b0, b1, b2 = _taps(b0, b1, b2, causal)
    toward, back = (ahead, shifted) if causal else (shifted, ahead)      # where the adjoint looks; where the forward looked
    gx = emu.fma(toward(b2, 2), toward(lam, 2), emu.fma(toward(b1, 1), toward(lam, 1), b0 * lam))
    one, two = np.ones(lam.shape[0], bool), np.ones(lam.shape[0], bool)
    if causal:
        one[:1] = two[:2] = False
    else:
        one[-1:] = two[-2:] = False
    zero = np.zeros_like(lam)
    g1 = np.where(one, lam * back(x, 1), zero)
    g2 = np.where(two, lam * back(x, 2), zero)
    h1 = np.where(one, -lam * back(y, 1), zero)
    h2 = np.where(two, -lam * back(y, 2), zero)
    return gx, lam * x, g1, g2, h1, h2
