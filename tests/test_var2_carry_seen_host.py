"""A test of the tests, on the CPU: would the suite see a var2_carry_1d that got the MATRIX half of the groups' maps wrong?

var2_carry_1d composes the groups' (E, P) as E = E_B + P_B E_A, P = P_B P_A across 64 lanes, 16 waves and sweeps of 1024 groups.
The numpy replay of the kernels' algebra (tests/var2_emulator.py) is run here with a wrong carry stage -- three mutants -- on every
case of the exact families (tests/var2_exact.py) and of the long-memory family (var2_cases / biquad_cases / cascade_cases
.LONG_MEMORY_CASES), in both directions, and every mutant has to FAIL the check the GPU tests apply to the kernels:
    exact cases     at least one differing sample behind the first carry that holds a product P_B E_A (the third group on)
    float cases     an error of at least 100 x the bar, on the forward and on the input's gradient
The last test records why these families exist: on the `near one` family (r <= 0.98, a group's P is 0.98^4096 = 1e-36) two of
the mutants change no bit.  Nothing here runs on a GPU."""
import functools

import numpy as np
import pytest

import biquad_cases
import biquad_emulator
import cascade_cases
import cascade_emulator
import var2_cases
import var2_emulator as emu
import var2_exact as exact

DIRECTIONS = [True, False]
GROUP = emu.T * emu.GROUP


def p_zeroed(aggregate):
    e0, e1, *p = aggregate
    return (e0, e1, *(np.zeros_like(c) for c in p))


def p_transposed(aggregate):
    e0, e1, p00, p01, p10, p11 = aggregate
    return (e0, e1, p00, p10, p01, p11)


def compose_reversed(A, B):
    return emu.compose(B, A)


MUTANTS = {"P zeroed": dict(mutate_aggregate=p_zeroed), "p01 and p10 swapped": dict(mutate_aggregate=p_transposed),
           "compose reversed in the carry's lane scan": dict(carry_compose=compose_reversed)}
CLEAN_SCAN = emu.tiled_scan


def name_of(causal):
    return "causal" if causal else "anticausal"


@pytest.fixture(params=list(MUTANTS))
def mutant(request, monkeypatch):
    """every scan of the replay, the ones inside the section's and the cascade's replay too, runs with this mutant"""
    monkeypatch.setattr(emu, "tiled_scan", functools.partial(CLEAN_SCAN, **MUTANTS[request.param]))
    return request.param


def behind_the_first_product(n, causal):
    """the samples of the third group on, in the order of the recurrence: their carry holds a P_B E_A"""
    full = -(-n // GROUP) * GROUP
    return np.s_[2 * GROUP:] if causal else np.s_[:full - 2 * GROUP]


def assert_differs(got, want, n, causal, what):
    where = behind_the_first_product(n, causal)
    differing = np.flatnonzero(np.asarray(got)[where] != np.asarray(want)[where])
    assert len(differing) > 0, f"{what}: the mutant gives the exact result"


def assert_far_above_the_bar(got, reference, what):
    want, err32, peak = reference
    err = var2_cases._figure(got, want, peak)
    bar = max(4 * err32, 1e-6)
    print(f"{what}: err/peak {err:.3e}, {err / bar:.0f} x the bar")
    assert err >= 100 * bar or np.isnan(err), f"{what}: the mutant is at {err / bar:.1f} x the bar only"


# ---- the exact cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("family", list(exact.FAMILIES))
@pytest.mark.parametrize("n", exact.LENGTHS)
def test_mutants_fail_the_exact_all_pole_cases(n, family, causal, mutant):
    x, a1, a2, _ = exact.case(n, family, causal)
    got = emu.tiled_forward(x[0], a1[0], a2[0], causal)
    assert_differs(got, exact.expected(n, family, causal)["out"][0], n, causal, f"{mutant}, {n} {family} {name_of(causal)}")


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("family", list(exact.FAMILIES))
@pytest.mark.parametrize("n", exact.LENGTHS[:2])
def test_mutants_fail_the_exact_biquad_cases(n, family, causal, mutant):
    signals = [s[0] for s in exact.biquad_case(n, family, causal)]
    got = biquad_emulator.tiled_forward(*signals[:6], causal)
    assert_differs(got, exact.biquad_expected(n, family, causal)["out"][0], n, causal, f"{mutant}, {n} biquad {family} {name_of(causal)}")


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", exact.LENGTHS[:2])
def test_mutants_fail_the_exact_cascade_cases(n, causal, mutant):
    x, sections, _ = exact.cascade_case(n, causal)
    got = cascade_emulator.tiled_forward(x[0], [tuple(c[0] for c in s) for s in sections], causal)
    assert_differs(got, exact.cascade_expected(n, causal)[0]["out"][0], n, causal, f"{mutant}, {n} cascade {name_of(causal)}")


# ---- the long-memory cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n,lines,kind", var2_cases.LONG_MEMORY_CASES)
def test_mutants_fail_the_long_memory_all_pole_cases(n, lines, kind, causal, mutant):
    x, a1, a2, g = var2_cases.case(n, lines, kind, causal)
    want = var2_cases.expected(n, lines, kind, causal)
    what = f"{mutant}, {n} {kind} {name_of(causal)}"
    assert_far_above_the_bar(emu.tiled_forward(x[0], a1[0], a2[0], causal)[None, :], want["out"], f"{what} out")
    assert_far_above_the_bar(emu.tiled_scan(g[0], a1[0], a2[0], not causal, True)[None, :], want["grad_x"], f"{what} grad_x")


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n,lines,kind", biquad_cases.LONG_MEMORY_CASES)
def test_mutants_fail_the_long_memory_biquad_cases(n, lines, kind, causal, mutant):
    signals = [s[0] for s in biquad_cases.case(n, lines, kind, causal)]
    want = biquad_cases.expected(n, lines, kind, causal)
    what = f"{mutant}, {n} biquad {kind} {name_of(causal)}"
    y = biquad_emulator.tiled_forward(*signals[:6], causal)
    assert_far_above_the_bar(y[None, :], want["out"], f"{what} out")
    # (the replay's gradients take a result as y: the reference's, so that grad_x shows the adjoint scan's own carry alone)
    gx = biquad_emulator.tiled_adjoint(*signals[:6], want["out"][0][0], signals[6], causal)[0]
    assert_far_above_the_bar(gx[None, :], want["grad_x"], f"{what} grad_x")


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n,lines,kind,K", cascade_cases.LONG_MEMORY_CASES)
def test_mutants_fail_the_long_memory_cascade_cases(n, lines, kind, K, causal, mutant):
    x, sections, g = cascade_cases.case(n, lines, kind, causal, K)
    one = [tuple(c[0] for c in s) for s in sections]
    want = cascade_cases.expected(n, lines, kind, causal, K)
    what = f"{mutant}, {n} cascade {kind} K={K} {name_of(causal)}"
    y = cascade_emulator.tiled_forward(x[0], one, causal)
    assert_far_above_the_bar(y[None, :], want["out"], f"{what} out")
    gx, _ = cascade_emulator.tiled_adjoint(x[0], one, want["out"][0][0], g[0], causal)
    assert_far_above_the_bar(gx[None, :], want["grad_x"], f"{what} grad_x")


# ---- the hole these families close --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("name", ["P zeroed", "p01 and p10 swapped"])
def test_near_one_at_8196_cannot_tell_a_wrong_matrix(name, causal):
    """r <= 0.98: every group's P is a matrix of zeros (0.98^4096 = 1e-36), so a carry stage that drops P or transposes it gives
    the bits of the right one -- on the forward and on the adjoint state.  Why the exact and the long-memory families exist"""
    x, a1, a2, g = var2_cases.case(8196, 1, "near one", causal)
    for signal, direction, adjoint in ((x[0], causal, False), (g[0], not causal, True)):
        clean = CLEAN_SCAN(signal, a1[0], a2[0], direction, adjoint)
        wrong = CLEAN_SCAN(signal, a1[0], a2[0], direction, adjoint, **MUTANTS[name])
        np.testing.assert_array_equal(wrong.view(np.uint32), clean.view(np.uint32))
