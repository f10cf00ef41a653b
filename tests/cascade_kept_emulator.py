"""The backward of a cascade whose forward kept every section's result (rf_var2_plan_backward_cascade_kept), replayed in numpy f32
on ONE line, on top of tests/var2_emulator.py, tests/biquad_emulator.py and tests/cascade_emulator.py.

From the last section down: the adjoint scan of section k (its tails, the carry and -- inside var2_adj_link_1d -- its final
stage), the gradient that enters section k - 1 formed on lam_k by the same launch, the five coefficient gradients of section k
from lam_k and the kept signals (var2_biquad_coef_1d); then the adjoint scan of section 0 and var2_biquad_grad_1d.

The adjoint link is the forward link with the direction flipped: `cascade_emulator.link_feed_forward` on lam_k with the taps
b1 and b2 read one and two samples further along the forward's direction.  The two samples of lam_k the taps reach beyond a tile
are the state that enters the tile in the adjoint scan's final stage (parts["enter"]), not the stored samples.  The shift drops
exactly the slots the forward masks -- b1[0], b2[0], b2[1] of a causal section -- so a NaN there is never referenced, and fills
with 0 where the tap would multiply lam outside the line, which is where link_feed_forward masks the taps of the flipped
direction."""
import numpy as np

import biquad_emulator as biquad
import cascade_emulator as cascade
import var2_emulator as emu
from biquad_loops import ahead, shifted

F = np.float32


def adjoint_link(lam, enter, b0, b1, b2, causal=True):
    """g_{k-1} of var2_adj_link_1d on lam (N,), section k's adjoint state; enter: parts["enter"] of the adjoint tiled_scan that
    formed lam; causal: the direction of the FORWARD section"""
    toward = ahead if causal else shifted
    b0, b1, b2 = (np.asarray(b, dtype=F) for b in (b0, b1, b2))
    return cascade.link_feed_forward(lam, enter, b0, toward(b1, 1), toward(b2, 2), not causal)


def coefficient_gradients(lam, x, y, causal=True):
    """(grad_b0, grad_b1, grad_b2, grad_a1, grad_a2) of var2_biquad_coef_1d: the products and selects of biquad_emulator.tiled_adjoint"""
    lam, x, y = (np.asarray(a, dtype=F) for a in (lam, x, y))
    back = shifted if causal else ahead
    one, two = np.ones(lam.shape[0], bool), np.ones(lam.shape[0], bool)
    if causal:
        one[:1] = two[:2] = False
    else:
        one[-1:] = two[-2:] = False
    zero = np.zeros_like(lam)
    return (lam * x, np.where(one, lam * back(x, 1), zero), np.where(two, lam * back(x, 2), zero),
            np.where(one, -lam * back(y, 1), zero), np.where(two, -lam * back(y, 2), zero))


def tiled_adjoint(x, sections, results, g, causal=True):
    """(grad_x, [(grad_b0, grad_b1, grad_b2, grad_a1, grad_a2) of section k]); results: every section's result, the K - 1 kept
    signals and then the cascade's (what cascade_emulator.tiled_forward puts into its `results`)"""
    K = len(sections)
    assert len(results) == K
    grads = [None] * K
    for k in range(K - 1, 0, -1):
        b0, b1, b2, a1, a2 = sections[k]
        parts = {}
        lam = emu.tiled_scan(g, a1, a2, not causal, True, parts)
        grads[k] = coefficient_gradients(lam, results[k - 1], results[k], causal)
        g = adjoint_link(lam, parts["enter"], b0, b1, b2, causal)
    g, *grads[0] = biquad.tiled_adjoint(x, *sections[0], results[0], g, causal)
    grads[0] = tuple(grads[0])
    return g, grads
