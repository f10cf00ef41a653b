"""A cascade of direct-form-I sections as the kernels form it, replayed in numpy f32 on ONE line, on top of
tests/var2_emulator.py and tests/biquad_emulator.py: var2_biquad_tails_1d in front, then per boundary between two sections
var2_carry_1d and var2_link_1d, then var2_carry_1d and var2_pass2_1d.

The link reruns section k's recurrence from the state that enters each tile (the emulator's parts["enter"]) and forms the
feed-forward part of section k + 1 on the result.  The two samples its taps reach beyond a tile are NOT the neighbouring tile's
stored samples: they are that entering state, (y1, y2) = what the recurrence takes for the samples one and two places before
the tile in its own direction.  `link_feed_forward` puts them where the shifted signal has the neighbour's samples."""
import numpy as np

import biquad_emulator as biquad
import var2_emulator as emu
from biquad_loops import ahead, shifted

F = np.float32
T = emu.T


def link_feed_forward(y, enter, b0, b1, b2, causal=True):
    """v of the next section on y (N,), the finished section's result; enter: parts["enter"] of the tiled_scan that formed y"""
    n = y.shape[0]
    y = np.asarray(y, dtype=F)
    y1, y2 = (e.reshape(-1) for e in enter)      # per tile, in the order of the recurrence
    tiles_full = y1.shape[0]
    b0, b1, b2 = biquad._taps(b0, b1, b2, causal)
    if causal:
        one, two = shifted(y, 1), shifted(y, 2)
        for j in range(-(-n // T)):
            t0 = j * T
            one[t0] = y1[j]
            two[t0] = y2[j]
            two[t0 + 1] = y1[j]
    else:
        one, two = ahead(y, 1), ahead(y, 2)
        for j in range(tiles_full):
            last = (tiles_full - 1 - j) * T + T - 1      # the tile's last sample in the line
            if last < n:
                one[last] = y1[j]
                two[last] = y2[j]
                two[last - 1] = y1[j]
    return emu.fma(b2, two, emu.fma(b1, one, b0 * y))


def tiled_forward(x, sections, causal=True, results=None):
    """the cascade's result on one line; results: a list that receives every section's result (what var2_link_keep_1d stores)"""
    v = biquad.feed_forward(x, *sections[0][:3], causal)
    for k, s in enumerate(sections):
        parts = {}
        y = emu.tiled_scan(v, s[3], s[4], causal, False, parts)
        if results is not None:
            results.append(y)
        if k + 1 < len(sections):
            v = link_feed_forward(y, parts["enter"], *sections[k + 1][:3], causal)
    return y


def tiled_adjoint(x, sections, out, g, causal=True):
    """(grad_x, [(grad_b0, grad_b1, grad_b2, grad_a1, grad_a2) of section k]) as rf_var2_plan_backward_cascade forms them: the
    results of all sections but the last from a rerun, the last one's from `out`"""
    ys = []
    if len(sections) > 1:
        tiled_forward(x, sections[:-1], causal, ys)
    ys.append(np.asarray(out, dtype=F))
    grads = [None] * len(sections)
    for k in range(len(sections) - 1, -1, -1):
        g, *grads[k] = biquad.tiled_adjoint(x if k == 0 else ys[k - 1], *sections[k], ys[k], g, causal)
        grads[k] = tuple(grads[k])
    return g, grads
