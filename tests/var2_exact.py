"""Exact cases of the time-varying second-order family: constant coefficients whose companion matrix M is an integer matrix of
finite order (or the running sum's), on inputs in {-1, 0, 1}.  Every state, every fma and every entry of a 2 x 2 map is then a
small integer, exact in f32 WHATEVER the order of operations, and the expected result is the integer one, bit for bit: the tests
that use these cases have no tolerance.  The state never decays, so a group's P reaches every later sample -- what no family
with a pole radius below 1 can show (tests/var2_cases.py).

    family        a1, a2    recurrence           impulse response            M^64, M^4096
    period 6      -1, +1    y = x + y1 - y2      1, 1, 0, -1, -1, 0, ...     M^4: not symmetric
    period 3      +1, +1    y = x - y1 - y2      1, -1, 0, ...               M^1: not symmetric
    running sum   -1,  0    y = x + y1           1, 1, 1, ...                [[1, 0], [1, 0]]: singular, not symmetric
(no family of period 2 or 4: its M^64 is the identity, which hides a transposition)

Reference: y[n] = sum_k h[(n - k) mod p] x[k] in int64 from p cumulative sums over the residue classes of k -- no loop over the
samples.  The anticausal scan is the same on the reversed line; with constant coefficients the adjoint state is the same
convolution of grad_out in the other direction (the masked slots meet a zero state; tests/test_var2_host.py pins all of it,
ends included, against the serial loops).  The section's taps and a cascade are integer expressions around it.

Everything returned is asserted to be below 2^24 in magnitude, products included: the density of the inputs falls with the
length, since a state walks like the square root of the number of non-zero inputs."""
import functools
import zlib

import numpy as np

from biquad_loops import ahead, shifted
from var2_cases import LONG

FAMILIES = {"period 6": (-1, 1), "period 3": (1, 1), "running sum": (-1, 0)}
IMPULSE = {"period 6": (1, 1, 0, -1, -1, 0), "period 3": (1, -1, 0), "running sum": (1,)}
TAPS = {"period 6": (1, -1, 0), "period 3": (1, 0, 1), "running sum": (1, 0, 1)}      # of the exact biquad cases
# four groups: the first non-trivial P_B E_A of either direction (an anticausal scan meets the 4-sample partial group first);
# 66 groups: the carry crosses a wave inside a sweep; LONG: 1026 groups, a second sweep
LENGTHS = [3 * 4096 + 4, 65 * 4096 + 4, LONG]
DENSITY = {LENGTHS[0]: 0.5, LENGTHS[1]: 0.05, LONG: 0.01}      # the share of non-zero inputs
LIMIT = 1 << 24
COEFFICIENTS = ("b0", "b1", "b2", "a1", "a2")


def scan(v, family, causal=True):
    """the all-pole scan of `family` on integers (..., N), int64"""
    v = np.asarray(v, dtype=np.int64)
    if not causal:
        return scan(v[..., ::-1], family, True)[..., ::-1]
    h = np.asarray(IMPULSE[family], dtype=np.int64)
    p = len(h)
    at = np.arange(v.shape[-1])
    y = np.zeros_like(v)
    for j in range(p):
        y += h[(at - j) % p] * np.cumsum(np.where(at % p == j, v, 0), axis=-1)
    return y


def within(*arrays):
    return all(int(np.max(np.abs(a))) < LIMIT for a in arrays)


def chain(x, g, sections, causal=True):
    """a cascade of sections [(family, (b0, b1, b2))] on integers, and its gradients: {name: int64 array}, the names those of
    cascade_cases.names(K), and "lam_k": the adjoint state of section k (checked against 2^24 with the rest)"""
    if not causal:
        return {k: v[..., ::-1] for k, v in chain(np.asarray(x)[..., ::-1], np.asarray(g)[..., ::-1], sections, True).items()}
    x, g = np.asarray(x, dtype=np.int64), np.asarray(g, dtype=np.int64)
    inputs, ys = [], []
    for family, (b0, b1, b2) in sections:
        inputs.append(x)
        x = scan(b0 * x + b1 * shifted(x, 1) + b2 * shifted(x, 2), family)
        ys.append(x)
    out = {"out": x}
    for k in range(len(sections) - 1, -1, -1):
        family, (b0, b1, b2) = sections[k]
        lam = scan(g, family, False)
        u, y = inputs[k], ys[k]
        out.update({f"grad_b0_{k}": lam * u, f"grad_b1_{k}": lam * shifted(u, 1), f"grad_b2_{k}": lam * shifted(u, 2),
                    f"grad_a1_{k}": -lam * shifted(y, 1), f"grad_a2_{k}": -lam * shifted(y, 2), f"lam_{k}": lam})
        g = b0 * lam + b1 * ahead(lam, 1) + b2 * ahead(lam, 2)
    out["grad_x"] = g
    return out


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(("exact",) + key).encode()))


def _constant(value, shape, masked, causal):
    a = np.full(shape, value, np.float32)
    a[(np.s_[..., :masked] if causal else np.s_[..., shape[-1] - masked:])] = np.nan
    return a


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def inputs(n, what):
    """(x, grad_out): (1, n) f32 in {-1, 0, 1}, seeded; shared and never written"""
    rng = _rng(n, what)
    d = DENSITY.get(n, 0.5)
    return _frozen(*(rng.choice(np.array([-1, 0, 1], np.float32), (1, n), p=[d / 2, 1 - d, d / 2]) for _ in range(2)))


def coefficient_signals(n, family, taps, causal):
    """(b0, b1, b2, a1, a2) as (1, n) f32, NaN in every slot the section masks"""
    (a1, a2), (b0, b1, b2) = FAMILIES[family], taps
    return _frozen(_constant(b0, (1, n), 0, causal), _constant(b1, (1, n), 1, causal), _constant(b2, (1, n), 2, causal),
                   _constant(a1, (1, n), 1, causal), _constant(a2, (1, n), 2, causal))


def _checked(results, what, may_exceed=False):
    """the int64 results as they are; all of them below 2^24, or (may_exceed) the ones that are not taken out and named"""
    left_out = sorted(name for name, a in results.items() if not within(a))
    assert may_exceed or not left_out, f"{what}: {left_out} reach 2^24"
    return {name: a for name, a in results.items() if name not in left_out and not name.startswith("lam_")}, left_out


# ---- the all-pole scan ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(n, family, causal):
    """(x, a1, a2, grad_out) for Var2Plan.execute / backward"""
    x, g = inputs(n, family)
    return (x, *coefficient_signals(n, family, (1, 0, 0), causal)[3:], g)


@functools.lru_cache(maxsize=None)
def expected(n, family, causal):
    """{"out", "grad_x", "grad_a1", "grad_a2"} -> int64 (1, n)"""
    x, g = inputs(n, family)
    r, _ = _checked(chain(x, g, [(family, (1, 0, 0))], causal), f"{n} {family}")
    return {"out": r["out"], "grad_x": r["grad_x"], "grad_a1": r["grad_a1_0"], "grad_a2": r["grad_a2_0"]}


# ---- the section ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def biquad_case(n, family, causal):
    """(x, b0, b1, b2, a1, a2, grad_out) for Var2Plan.execute_biquad / backward_biquad"""
    x, g = inputs(n, ("biquad", family))
    return (x, *coefficient_signals(n, family, TAPS[family], causal), g)


@functools.lru_cache(maxsize=None)
def biquad_expected(n, family, causal):
    """biquad_cases.NAMES -> int64 (1, n)"""
    x, g = inputs(n, ("biquad", family))
    r, _ = _checked(chain(x, g, [(family, TAPS[family])], causal), f"{n} biquad {family}")
    return {"out": r["out"], "grad_x": r["grad_x"], **{f"grad_{c}": r[f"grad_{c}_0"] for c in COEFFICIENTS}}


# ---- the cascade: two sections of DIFFERENT periods (two of the same period resonate and grow linearly) ---------------------------
CASCADE = [("period 6", (1, -1, 0)), ("period 3", (1, 0, 1))]


@functools.lru_cache(maxsize=None)
def cascade_case(n, causal):
    """(x, sections, grad_out) for Var2Plan.execute_cascade / backward_cascade"""
    x, g = inputs(n, "cascade")
    return x, tuple(coefficient_signals(n, family, taps, causal) for family, taps in CASCADE), g


@functools.lru_cache(maxsize=None)
def cascade_expected(n, causal):
    """(cascade_cases.names(2) -> int64 (1, n), the names left out because they reach 2^24); "out" is never left out"""
    x, g = inputs(n, "cascade")
    r, left_out = _checked(chain(x, g, CASCADE, causal), f"{n} cascade", True)
    assert "out" in r and "grad_x" in r, left_out
    return r, left_out


# ---- the comparison -----------------------------------------------------------------------------------------------------------------
def assert_equal(got, want, what, causal):
    """got (lines, n) equals the integers, no tolerance (a NaN differs).  A mismatch names its first sample in the order of the
    recurrence: by tile (64 samples: the lane scan of a group), group (4096: the carry's lane scan; 64 groups: its fold of the
    waves' totals) and sweep (1024 groups: the state the carry keeps between sweeps)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    n = got.shape[-1]
    full = -(-n // 4096) * 4096
    for line, (a, b) in enumerate(zip(got, want)):
        differing = np.flatnonzero(a != b)
        if len(differing):
            at = int(differing[0] if causal else differing[-1])
            k = at if causal else full - 1 - at      # an anticausal scan runs the padded line reversed
            raise AssertionError(f"{what}: line {line}, {len(differing)} of {n} samples differ; the first in the order of the recurrence is "
                                 f"sample {at} -- place {k}: tile {k // 64}, group {k // 4096}, wave {k // (64 * 4096)}, sweep "
                                 f"{k // (1024 * 4096)} -- got {a[at]!r}, want {int(b[at])}")
