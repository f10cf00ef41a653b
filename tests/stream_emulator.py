"""One chunk of a cascade on frames with a state, as the STREAM instances of the frames kernels form it, replayed in numpy f32 on
ONE line: tests/cascade_emulator.py's forward (tests/cascade_kept_emulator.py's kept results) plus the border terms.  Every
section keeps its masks by position; the entering state is folded into the two first samples of its v, in the order of the
recurrence (causal: samples 0 and 1; anticausal: n - 1 and n - 2), with the chunk's unmasked coefficients:

    v[0] = fma(b2[0], hx2, fma(b1[0], hx1, b0[0] * src[0]))          v[0] = fma(-a1[0], hy1, fma(-a2[0], hy2, v[0]))
    v[1] = fma(b2[1], hx1, fma(b1[1], src[0], b0[1] * src[1]))       v[1] = fma(-a2[1], hy1, v[1])

src the section's input, (hx1, hx2) pair k and (hy1, hy2) pair k + 1 of the state.  The masked tiled scan from zero then runs on
that v unchanged.  The leaving state is the two last samples of x and of every section's result.  `sections`: K tuples of the
chunk's five coefficients at audio rate (tests/frames_loops.py's f32 expansion of the chunk's frames)."""
import numpy as np

import biquad_emulator as biquad
import cascade_emulator
import var2_emulator as emu

F = np.float32


def fold(v, src, section, hx, hy, causal=True):
    """v with the entering state folded into its two first samples"""
    b0, b1, b2, a1, a2 = (np.asarray(c, dtype=F) for c in section)
    n = v.shape[0]
    i0, i1 = (0, 1) if causal else (n - 1, n - 2)
    hx1, hx2, hy1, hy2 = F(hx[0]), F(hx[1]), F(hy[0]), F(hy[1])
    v0 = emu.fma(b2[i0], hx2, emu.fma(b1[i0], hx1, b0[i0] * src[i0]))
    v1 = emu.fma(b2[i1], hx1, emu.fma(b1[i1], src[i0], b0[i1] * src[i1]))
    v = v.copy()
    v[i0] = emu.step2(a1[i0], a2[i0], v0, hy1, hy2)
    v[i1] = emu.fma(-a2[i1], hy1, v1)
    return v


def last_two(y, causal):
    return (y[-1], y[-2]) if causal else (y[0], y[1])


def tiled_forward(x, sections, state=None, causal=True, results=None):
    """(the chunk's result, the state that leaves as (K + 1, 2) f32); state None: nothing is folded (the call with state_in null);
    results: a list that receives every section's result (what the keep instance of the link stores)"""
    x = np.asarray(x, dtype=F)
    K = len(sections)
    leaving = np.empty((K + 1, 2), F)
    leaving[0] = last_two(x, causal)
    src = x
    v = biquad.feed_forward(x, *sections[0][:3], causal)
    for k, s in enumerate(sections):
        if state is not None:
            v = fold(v, src, s, state[k], state[k + 1], causal)
        parts = {}
        y = emu.tiled_scan(v, s[3], s[4], causal, False, parts)
        leaving[k + 1] = last_two(y, causal)
        if results is not None:
            results.append(y)
        if k + 1 < K:
            v = cascade_emulator.link_feed_forward(y, parts["enter"], *sections[k + 1][:3], causal)
            src = y
    return y, leaving


def history_gradients(lam, src, y, hx, hy, causal=True):
    """the five per-sample coefficient gradients with the history where the forward read it: the products of
    cascade_kept_emulator.coefficient_gradients, nothing masked; hx, hy None: that function (zeros enter, the slots selected to +0)"""
    import cascade_kept_emulator
    if hx is None:
        return cascade_kept_emulator.coefficient_gradients(lam, src, y, causal)
    lam, src, y = (np.asarray(a, dtype=F) for a in (lam, src, y))

    def back(s, h, d):      # s[n - d] (anticausal: s[n + d]) with the history beyond the line
        if causal:
            return np.concatenate([[F(h[1]), F(h[0])], s])[2 - d:s.shape[0] + 2 - d]
        return np.concatenate([s, [F(h[0]), F(h[1])]])[d:s.shape[0] + d]
    return (lam * src, lam * back(src, hx, 1), lam * back(src, hx, 2), -lam * back(y, hy, 1), -lam * back(y, hy, 2))


def tiled_adjoint(x, sections, results, g, state=None, grad_state_out=None, causal=True):
    """(grad_x, [(grad_b0, .. grad_a2) of section k, per sample], grad_state_in (K + 1, 2)) as the STREAM instances of the backward
    form them: tests/cascade_kept_emulator.py's backward with the gradient of the leaving pairs added in f32 to the two last samples
    of the gradient each signal receives, the history in the coefficient gradients, and grad_state_in from lam_k at the forward's
    two first samples -- feedback part (fma(-a1[0], lam[0], -(a2[1] * lam[1])), -(a2[0] * lam[0])) to pair k + 1, added to what
    section k + 1 stored there; feed-forward part (fma(b1[0], lam[0], b2[1] * lam[1]), b2[0] * lam[0]) stored to pair k"""
    import cascade_kept_emulator as kept_emulator
    from biquad_loops import ahead, shifted
    K, n = len(sections), np.asarray(x).shape[0]
    last = (n - 1, n - 2) if causal else (0, 1)
    first = (0, 1) if causal else (n - 1, n - 2)
    G = np.zeros((K + 1, 2), F) if grad_state_out is None else np.asarray(grad_state_out, dtype=F)
    gsi = np.zeros((K + 1, 2), F)
    grads = [None] * K

    def add(v, pair):
        v = np.array(v, dtype=F)
        v[last[0]] = v[last[0]] + pair[0]
        v[last[1]] = v[last[1]] + pair[1]
        return v

    def entering(k, lam):
        b0, b1, b2, a1, a2 = (np.asarray(c, dtype=F) for c in sections[k])
        l0, l1 = lam[first[0]], lam[first[1]]
        fb = (emu.fma(-a1[first[0]], l0, -(a2[first[1]] * l1)), -(a2[first[0]] * l0))
        if k == K - 1:
            gsi[k + 1] = fb
        else:
            gsi[k + 1] = (gsi[k + 1, 0] + fb[0], gsi[k + 1, 1] + fb[1])
        gsi[k] = (emu.fma(b1[first[0]], l0, b2[first[1]] * l1), b2[first[0]] * l0)
    g = add(g, G[K])
    for k in range(K - 1, 0, -1):
        b0, b1, b2, a1, a2 = sections[k]
        parts = {}
        lam = emu.tiled_scan(g, a1, a2, not causal, True, parts)
        grads[k] = history_gradients(lam, results[k - 1], results[k], None if state is None else state[k], None if state is None else state[k + 1], causal)
        entering(k, lam)
        g = add(kept_emulator.adjoint_link(lam, parts["enter"], b0, b1, b2, causal), G[k])
    b0, b1, b2, a1, a2 = sections[0]
    lam = emu.tiled_scan(g, a1, a2, not causal, True)
    grads[0] = history_gradients(lam, x, results[0], None if state is None else state[0], None if state is None else state[1], causal)
    entering(0, lam)
    t0, t1, t2 = biquad._taps(b0, b1, b2, causal)
    toward = ahead if causal else shifted
    gx = emu.fma(toward(t2, 2), toward(lam, 2), emu.fma(toward(t1, 1), toward(lam, 1), t0 * lam))
    return add(gx, G[0]), grads, gsi
