"""Serial loops of a cascade of time-varying direct-form-I sections (rf_var2_plan_execute_cascade / _backward_cascade), the
yardsticks of tests/test_cascade_host.py and tests/test_gpu_cascade_signal.py, chained from tests/biquad_loops.py in the
arithmetic of `dtype`.  `sections` is a sequence of K tuples (b0, b1, b2, a1, a2), arrays shaped like x, (N,) or (L, N); every
section runs in the one direction `causal`, section k + 1 on the result of section k.

    forward     y_0 = biquad(x, sections[0]),  y_k = biquad(y_{k-1}, sections[k]);  returns [y_0, ..., y_{K-1}]
    adjoint     from the last section to the first: biquad_loops.adjoint with x = y_{k-1}, y = y_k, g = g_k; g_{k-1} = its grad_x

segmented=True: ONE long line whose sections' a1, a2 each cut it into segments (biquad_loops.segmented_*)."""
import numpy as np

import biquad_loops as loops


def forward(x, sections, causal=True, dtype=np.float64, segmented=False):
    """the results of all sections, the cascade's own last"""
    run = loops.segmented_forward if segmented else loops.forward
    ys = []
    for s in sections:
        x = run(x, *s, causal, dtype)
        ys.append(x)
    return ys


def adjoint(x, sections, ys, g, causal=True, dtype=np.float64, segmented=False):
    """(grad_x, [(grad_b0, grad_b1, grad_b2, grad_a1, grad_a2) of section k]); ys: forward's results in `dtype`"""
    run = loops.segmented_adjoint if segmented else loops.adjoint
    grads = [None] * len(sections)
    for k in range(len(sections) - 1, -1, -1):
        g, *grads[k] = run(x if k == 0 else ys[k - 1], *sections[k], ys[k], g, causal, dtype)
        grads[k] = tuple(grads[k])
    return g, grads
