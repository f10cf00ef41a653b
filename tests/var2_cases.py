"""The cases tests/test_var2_host.py (the numpy emulator) and tests/test_gpu_var2_signal.py (the kernels) share: seeded inputs, the
coefficient families, the f64 references with the f32 serial loops' error figures, and the bar.

The bar is the varying family's: max abs error over the peak <= max(4 x the same figure of the numpy f32 serial loop, 1e-6),
against the f64 loop.  The peak is the input's for the forward, the reference's own for a gradient (tests/var_grad_cases.py).

Families (a1 = -2 r cos(theta), a2 = r^2: a resonator whose pole radius and angle move):
  resonator   r[n] inside [0.5, 0.98], moving slowly; theta[n] a slow random walk inside [0.2, pi - 0.2]
  near one    the same with r inside [0.9, 0.98]
  sprinkled   the resonator with decoupling zeros every 200..600 samples: a1[s-1] = a1[s] = 0 and a2[s-2 .. s+1] = 0 cut the line
              before sample s for a scan of either direction
  long memory       the resonator with r inside [0.998, 0.9995]: a group of 4096 samples shrinks the state by 3e-4 .. 0.13 only, so
                    the matrix half of the groups' maps reaches the result (with r <= 0.98 it is 0.98^4096 = 1e-36, a zero).  Above
                    0.9995 the f32 tiled algebra itself loses to the f32 serial loop.  Not in KINDS: LONG_MEMORY_CASES
  long memory, cut  the same with decoupling zeros every 20,000..40,000 samples, for the long line and its segmented loops
Every coefficient the scan masks holds NaN."""
import functools
import zlib

import numpy as np

import var2_loops as loops

LENGTHS = [4, 60, 64, 68, 4092, 4096, 4100, 8196]
LONG = 1025 * 4096 + 4       # 4,198,404 samples: 1026 groups, two sweeps of var2_carry_1d
KINDS = ["resonator", "near one", "sprinkled"]
# (lines, length, stride): rows further apart than they are long
LINE_CASES = [(3, 4100, 4112), (70, 196, 200)]
MEMORY_LENGTHS = [3 * 4096 + 4, 65 * 4096 + 4]      # 4 groups: the first P_B E_A of either direction; 66 groups: a second wave
# (n, lines, kind) of the long-memory family; both directions each
LONG_MEMORY_CASES = [(n, 1, "long memory") for n in MEMORY_LENGTHS] + [(LONG, 1, "long memory, cut")]
# The seed of every long-memory case, chosen on the CPU so that the numpy replay of the kernels (tests/var2_emulator.py, not the
# kernels) is at or below HALF the bar on the forward and all three gradients -- the f32 serial loop's error is itself one noisy
# draw; tests/test_var2_host.py asserts it.  {(n, kind, causal): seed}      the replay's worst err / f32 serial loop's (bar: 4)
LONG_MEMORY_SEEDS = {
    (MEMORY_LENGTHS[0], "long memory", True): 2,         # 1.20 (grad_x)       seeds 0, 1: out 4.48, grad_x 2.42
    (MEMORY_LENGTHS[0], "long memory", False): 2,        # 0.96 (grad_a1)      seeds 0, 1: grad_a2 2.58, out 3.26
    (MEMORY_LENGTHS[1], "long memory", True): 7,         # 1.85 (out)          seeds 0 .. 6: 2.24 .. 3.95
    (MEMORY_LENGTHS[1], "long memory", False): 10,       # 1.92 (grad_a1)      seeds 0 .. 9: 2.11 .. 4.34
    (LONG, "long memory, cut", True): 3,                 # 1.97 (grad_a2)      seeds 0 .. 2: 2.44 .. 3.70
    (LONG, "long memory, cut", False): 5,                # 1.94 (grad_x)       seed 0: 2.00, at the edge; 1 .. 3: 2.39 .. 4.77; 4: a cut at a sweep
}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def coefficients(kind, shape, rng):
    """(a1, a2) of a family, f32, nothing masked yet"""
    n = shape[-1]
    theta = 1.2 + np.cumsum(rng.normal(0.0, 0.01, shape), axis=-1)
    theta = 0.2 + np.abs((theta - 0.2) % (2 * (np.pi - 0.4)) - (np.pi - 0.4))      # reflected into [0.2, pi - 0.2]
    lo, hi = {"near one": (0.9, 0.98), "long memory": (0.998, 0.9995), "long memory, cut": (0.998, 0.9995)}.get(kind, (0.5, 0.98))
    phase = rng.random(shape[:-1] + (1,)) * 6.0 + np.cumsum(rng.normal(0.0, 0.02, shape), axis=-1)
    r = lo + (hi - lo) * (0.5 + 0.5 * np.sin(phase))
    a1 = (-2.0 * r * np.cos(theta)).astype(np.float32)
    a2 = (r * r).astype(np.float32)
    if kind in ("sprinkled", "long memory, cut") and n > 8:
        lo, hi = (200, 600) if kind == "sprinkled" else (20000, 40000)
        cuts = np.cumsum(rng.integers(lo, hi + 1, n // lo + 1))
        cuts = cuts[(cuts >= 2) & (cuts < n - 1)]
        for k in (-1, 0):
            a1[..., cuts + k] = 0.0
        for k in (-2, -1, 0, 1):
            a2[..., cuts + k] = 0.0
    return a1, a2


@functools.lru_cache(maxsize=None)
def case(n, lines, kind, causal):
    """(x, a1, a2, grad_out) as (lines, n) f32 arrays, seeded; shared and never written"""
    rng = _rng(n, lines, kind, "seed", LONG_MEMORY_SEEDS[n, kind, causal]) if kind.startswith("long memory") else _rng(n, lines, kind)
    shape = (lines, n)
    x = (rng.random(shape) * 2 - 1).astype(np.float32)
    g = (rng.random(shape) * 2 - 1).astype(np.float32)
    a1, a2 = coefficients(kind, shape, rng)
    if kind == "long memory, cut":
        assert_state_crosses_the_sweeps(a1[0], a2[0])
    if causal:
        a1[:, :1] = np.nan
        a2[:, :2] = np.nan
    else:
        a1[:, -1:] = np.nan
        a2[:, -2:] = np.nan
    for a in (x, a1, a2, g):
        a.setflags(write=False)
    return x, a1, a2, g


def assert_state_crosses_the_sweeps(a1, a2):
    """no decoupling zero within 8192 samples of where var2_carry_1d goes from one sweep of 1024 groups to the next: sample
    1024 * 4096 of a causal scan, (groups - 1024) * 4096 of an anticausal one (whose padded line runs reversed)"""
    n = a1.shape[0]
    groups = -(-n // 4096)
    assert groups > 1024
    cuts = np.flatnonzero((a1 == 0) & (a2 == 0))
    assert len(cuts) > 50
    for edge in (1024 * 4096, (groups - 1024) * 4096):
        assert np.min(np.abs(cuts - edge)) > 8192, f"a cut {np.min(np.abs(cuts - edge))} samples from the sweep boundary at {edge}"


def _figure(got, want, peak):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want))) / peak


@functools.lru_cache(maxsize=None)
def expected(n, lines, kind, causal):
    """the f64 references and the f32 serial loops' figures:
    {"out", "grad_x", "grad_a1", "grad_a2"} -> (reference, err32 / peak, peak)"""
    x, a1, a2, g = case(n, lines, kind, causal)
    long = n >= LONG
    results = {}
    for dtype in (np.float64, np.float32):
        if long:
            y = loops.segmented_forward(x[0], a1[0], a2[0], causal, dtype)[None, :]
            grads = [r[None, :] for r in loops.segmented_adjoint(a1[0], a2[0], y[0], g[0], causal, dtype)]
        else:
            y = loops.forward(x, a1, a2, causal, dtype)
            grads = list(loops.adjoint(a1, a2, y, g, causal, dtype))
        results[dtype] = dict(zip(("out", "grad_x", "grad_a1", "grad_a2"), [y] + grads))
    out = {}
    for name, want in results[np.float64].items():
        peak = float(np.max(np.abs(x))) if name == "out" else max(float(np.max(np.abs(want))), 1e-30)
        out[name] = (want, _figure(results[np.float32][name], want, peak), peak)
    return out


def assert_under_half_the_bar(got, reference, what):
    """the condition a seed of a long-memory case is chosen by, on the numpy replay: err <= max(2 x f32 serial loop, 5e-7)"""
    want, err32, peak = reference
    got = np.asarray(got)
    assert got.shape == want.shape and not np.isnan(got).any(), what
    err = _figure(got, want, peak)
    ratio = err / max(err32, 1e-30)
    print(f"{what}: err/peak {err:.3e}, f32 serial loop {err32:.3e}, ratio {ratio:.2f}")
    assert err <= max(2 * err32, 5e-7), f"{what}: err/peak {err:.3e} above half the bar (f32 serial loop: {err32:.3e})"
    return ratio


RATIOS = {}      # what -> the worst err / err32 seen (printed by the tests that fill it)


def assert_under_bar(got, reference, what):
    """`reference`: an entry of expected()"""
    want, err32, peak = reference
    got = np.asarray(got)
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    assert not np.isnan(got).any(), f"{what}: NaN in the result"
    err = _figure(got, want, peak)
    bar = max(4 * err32, 1e-6)
    ratio = err / max(err32, 1e-30)
    print(f"{what}: err/peak {err:.3e}, f32 serial loop {err32:.3e}, ratio {ratio:.2f}")
    assert err <= bar, f"{what}: err/peak {err:.3e} above the bar {bar:.3e} (f32 serial loop: {err32:.3e})"
    return ratio
