"""CPU tests of the time-varying direct-form-I section (rf_var2_plan_execute_biquad / _backward_biquad): the loops of
tests/biquad_loops.py pinned against scipy.signal.lfilter and central differences, the numpy replay of the kernels
(tests/biquad_emulator.py) under the GPU tests' bar on every case the GPU tests use, the two exact identities of the operator, the
exported symbols, and every refusal of a call in its documented order on a host-only plan.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest

import biquad_cases as cases
import biquad_emulator as emu
import biquad_loops as loops
import var2_cases
import var2_emulator
import var2_exact as exact
import recfilter_amd as rfa
from recfilter_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = [True, False]
NEW_SYMBOLS = ["rf_var2_plan_execute_biquad", "rf_var2_plan_execute_biquad_timed", "rf_var2_plan_backward_biquad",
               "rf_var2_plan_backward_biquad_timed", "rf_var2_plan_biquad_num_kernels", "rf_var2_plan_backward_biquad_num_kernels",
               "rf_var2_plan_backward_biquad_bytes"]


def name_of(causal):
    return "causal" if causal else "anticausal"


def host_plan(length, lines=1, causal=True, stride=None):
    return rfa.Var2Plan(length, lines=lines, causal=causal, device=capi.RF_DEVICE_HOST_ONLY, stride=stride)


# ---- the loops ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
def test_f64_loop_is_lfilter_for_constant_coefficients(causal):
    """constant coefficients: the section is scipy.signal.lfilter([b0, b1, b2], [1, a1, a2]); anticausal: on the signal reversed"""
    from scipy.signal import lfilter
    n = 300
    rng = np.random.default_rng(300)
    x = rng.random((2, n)) * 2 - 1
    b, a = [0.8, -0.9, 0.45], [1.0, -1.2, 0.81]
    full = [np.full((2, n), c) for c in b + a[1:]]
    got = loops.forward(x, *full, causal, np.float64)
    want = lfilter(b, a, x, axis=-1) if causal else lfilter(b, a, x[:, ::-1], axis=-1)[:, ::-1]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * float(np.max(np.abs(want))))


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_adjoint_loops_against_central_differences(causal):
    """the directional derivative of L = sum(g * y) along random directions in x and in each coefficient signal, f64"""
    n, h = 68, 1e-6
    rng = np.random.default_rng(168 + causal)
    x, g = (rng.random((2, n)) * 2 - 1 for _ in range(2))
    a1, a2 = (np.asarray(a, dtype=np.float64) for a in cases.var2_cases.coefficients("resonator", (2, n), rng))
    b0, b1, b2 = (np.asarray(b, dtype=np.float64) for b in cases.taps((2, n), rng))
    signals = [x, b0, b1, b2, a1, a2]

    def loss(s):
        return float(np.sum(g * loops.forward(*s, causal, np.float64)))
    y = loops.forward(*signals, causal, np.float64)
    grads = loops.adjoint(*signals, y, g, causal, np.float64)
    for i, grad in enumerate(grads):
        d = rng.random((2, n)) * 2 - 1
        up, down = list(signals), list(signals)
        up[i], down[i] = signals[i] + h * d, signals[i] - h * d
        assert abs((loss(up) - loss(down)) / (2 * h) - float(np.sum(grad * d))) < 1e-6, f"signal {i}"
        assert np.any(grad != 0)
    one, two = (np.s_[:, :1], np.s_[:, :2]) if causal else (np.s_[:, -1:], np.s_[:, -2:])
    assert np.all(grads[2][one] == 0) and np.all(grads[3][two] == 0) and np.all(grads[4][one] == 0) and np.all(grads[5][two] == 0)


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_segmented_loops_are_the_loops(causal):
    signals = cases.case(8196, 1, "sprinkled", causal)
    y = loops.forward(*signals[:6], causal)
    one = [s[0] for s in signals]
    np.testing.assert_allclose(loops.segmented_forward(*one[:6], causal), y[0], rtol=0, atol=1e-12)
    for got, want in zip(loops.segmented_adjoint(*one[:6], y[0], one[6], causal), loops.adjoint(*signals[:6], y, signals[6], causal)):
        np.testing.assert_allclose(got, want[0], rtol=0, atol=1e-10)


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_a_nan_in_a_masked_slot_reaches_nothing(causal):
    signals = cases.case(68, 1, "resonator", causal)
    assert [int(np.isnan(s).sum()) for s in signals] == [0, 0, 1, 2, 1, 2, 0]
    y = loops.forward(*signals[:6], causal)
    assert not np.isnan(y).any() and not any(np.isnan(r).any() for r in loops.adjoint(*signals[:6], y, signals[6], causal))
    one = [s[0] for s in signals]
    ye = emu.tiled_forward(*one[:6], causal)
    assert not np.isnan(ye).any() and not any(np.isnan(r).any() for r in emu.tiled_adjoint(*one[:6], ye, one[6], causal))


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [5, 4101])
def test_padding_rule_of_biquad_scan(n, causal):
    """zeros in all six signals behind the end of a causal section, before the start of an anticausal one: the real samples and
    their gradients are the unpadded section's"""
    rng = np.random.default_rng(n)
    x, g = (rng.random(n) * 2 - 1 for _ in range(2))
    a1, a2 = (np.asarray(a, dtype=np.float64) for a in cases.var2_cases.coefficients("resonator", (n,), rng))
    b = [np.asarray(t, dtype=np.float64) for t in cases.taps((n,), rng)]
    pad = -n % 4
    where = (0, pad) if causal else (pad, 0)
    keep = np.s_[:n] if causal else np.s_[pad:]
    signals = [x, *b, a1, a2]
    padded = [np.pad(s, where) for s in signals]
    y = loops.forward(*signals, causal)
    py = loops.forward(*padded, causal)
    np.testing.assert_array_equal(py[keep], y)
    for got, want in zip(loops.adjoint(*padded, py, np.pad(g, where), causal), loops.adjoint(*signals, y, g, causal)):
        np.testing.assert_array_equal(got[keep], want)


# ---- the emulator ---------------------------------------------------------------------------------------------------------------
GPU_CASES = ([(n, 1, kind) for n in cases.LENGTHS for kind in cases.KINDS] + [(n, lines, "resonator") for lines, n, _ in cases.LINE_CASES]
             + [(cases.LONG, 1, "sprinkled")] + cases.LONG_MEMORY_CASES)


def replay(signals, causal):
    lines, n = signals[0].shape
    got = {name: np.empty((lines, n), np.float32) for name in cases.NAMES}
    for l in range(lines):
        one = [s[l] for s in signals]
        y = emu.tiled_forward(*one[:6], causal)
        for name, r in zip(cases.NAMES, (y, *emu.tiled_adjoint(*one[:6], y, one[6], causal))):
            got[name][l] = r
    return got


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n,lines,kind", GPU_CASES)
def test_emulator_under_the_bar_on_every_gpu_case(n, lines, kind, causal):
    """what makes the GPU tests ones the algebra itself passes: forward and all six gradients of the numpy f32 replay"""
    want = cases.expected(n, lines, kind, causal)
    got = replay(cases.case(n, lines, kind, causal), causal)
    for name in cases.NAMES:
        cases.assert_under_bar(got[name], want[name], f"emulator {n} x {lines} {kind} {name_of(causal)} {name}")


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n,lines,kind", cases.LONG_MEMORY_CASES)
def test_emulator_under_half_the_bar_on_every_long_memory_case(n, lines, kind, causal):
    """the condition the seeds of cases.LONG_MEMORY_SEEDS were chosen by"""
    assert set(cases.LONG_MEMORY_SEEDS) == {(n, kind, c) for n, _, kind in cases.LONG_MEMORY_CASES for c in DIRECTIONS}
    want = cases.expected(n, lines, kind, causal)
    got = replay(cases.case(n, lines, kind, causal), causal)
    for name in cases.NAMES:
        var2_cases.assert_under_half_the_bar(got[name], want[name], f"emulator {n} x {lines} {kind} {name_of(causal)} {name}")


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("family", list(exact.FAMILIES))
@pytest.mark.parametrize("n", exact.LENGTHS[:2])
def test_emulator_is_exact_on_every_exact_gpu_case(n, family, causal):
    """integer taps in front of the integer rotations of tests/var2_exact.py: the replay gives the integers, forward and all six
    gradients, no tolerance (the closed form itself is pinned against the loops in tests/test_var2_host.py)"""
    want = exact.biquad_expected(n, family, causal)
    got = replay(exact.biquad_case(n, family, causal), causal)
    assert tuple(want) == cases.NAMES
    for name in cases.NAMES:
        np.testing.assert_array_equal(got[name], want[name], name)


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [68, 4100, 8196])
def test_unit_taps_give_the_all_pole_scan_in_bits(n, causal):
    x, _, _, _, a1, a2, _ = (s[0] for s in cases.case(n, 1, "resonator", causal))
    one, zero = np.ones(n, np.float32), np.zeros(n, np.float32)
    got = emu.tiled_forward(x, one, zero, zero, a1, a2, causal)
    np.testing.assert_array_equal(got.view(np.uint32), var2_emulator.tiled_forward(x, a1, a2, causal).view(np.uint32))


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [68, 4100, 8196])
def test_zero_feedback_gives_the_feed_forward_part_in_bits(n, causal):
    x, b0, b1, b2, _, _, _ = (s[0] for s in cases.case(n, 1, "resonator", causal))
    zero = np.zeros(n, np.float32)
    got = emu.tiled_forward(x, b0, b1, b2, zero, zero, causal)
    np.testing.assert_array_equal(got.view(np.uint32), emu.feed_forward(x, b0, b1, b2, causal).view(np.uint32))
    # and the expression itself, written out for one sample in the middle of the line
    i = n // 2
    s = 1 if causal else -1
    f = var2_emulator.fma
    want = f(b2[i:i + 1], x[i - 2 * s:i - 2 * s + 1], f(b1[i:i + 1], x[i - s:i - s + 1], b0[i:i + 1] * x[i:i + 1]))
    assert got[i] == want[0]


# ---- symbols --------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_typed():
    header = open(os.path.join(ROOT, "include", "recfilter_amd.h")).read()
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTED_SYMBOLS
        assert re.search(r"\b" + name + r"\(", header), f"{name} is not declared in recfilter_amd.h"
        assert getattr(L, name).argtypes is not None, f"{name} has no argument types"
    assert L.rf_var2_plan_backward_biquad_bytes.restype is ctypes.c_size_t
    assert len(L.rf_var2_plan_execute_biquad.argtypes) == 9 and len(L.rf_var2_plan_backward_biquad.argtypes) == 16
    assert capi.RF_ABI == 3 and b"abi 3" in L.rf_version()
    assert "biquad_scan" in rfa.__all__ and callable(rfa.biquad_scan)
    for method in ("execute_biquad", "execute_biquad_timed", "backward_biquad", "backward_biquad_timed", "apply_biquad"):
        assert callable(getattr(rfa.Var2Plan, method))


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("length,lines,stride", [(4, 1, 4), (4096, 1, 4096), (4100, 3, 4112), (1 << 30, 1, 1 << 30)])
def test_queries_of_host_only_plans(length, lines, stride, causal):
    tiles = -(-length // 64)
    groups = -(-tiles // 64)
    with host_plan(length, lines, causal, stride) as plan:
        assert plan.biquad_num_kernels == 3
        assert plan.backward_biquad_num_kernels == 4
        assert plan.backward_biquad_bytes == 4 * ((lines - 1) * stride + length)
        assert plan.workspace_bytes == 4 * lines * (6 * (tiles + groups) + 2 * groups)      # unchanged
        assert plan.num_kernels == 3 and plan.backward_num_kernels(True) == 4
    null = ctypes.c_void_p()
    L = capi.lib()
    assert L.rf_var2_plan_biquad_num_kernels(null) == 0 and L.rf_var2_plan_backward_biquad_num_kernels(null) == 0
    assert L.rf_var2_plan_backward_biquad_bytes(null) == 0


def test_host_only_plan_refuses_to_run_and_a_short_report_is_refused_first():
    with host_plan(4096) as plan:
        for call in (lambda: plan.execute_biquad(*[None] * 6), lambda: plan.execute_biquad_timed(*[None] * 6),
                     lambda: plan.backward_biquad(*[None] * 8), lambda: plan.backward_biquad_timed(*[None] * 8)):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == capi.RF_ERR_HIP and "host-only" in str(e.value)
        null, ms = ctypes.c_void_p(), (ctypes.c_float * 3)()
        L = capi.lib()
        assert L.rf_var2_plan_execute_biquad_timed(plan._h, *[null] * 8, ms, None, 2) == capi.RF_ERR_INVALID_ARG
        assert b"ms_out" in L.rf_last_error_string()
        assert L.rf_var2_plan_backward_biquad_timed(plan._h, *[null] * 15, ms, None, 3) == capi.RF_ERR_INVALID_ARG
        assert b"ms_out" in L.rf_last_error_string()
    assert L.rf_var2_plan_execute_biquad(*[null] * 9) == capi.RF_ERR_INVALID_ARG and L.rf_last_error_string()
    assert L.rf_var2_plan_backward_biquad(*[null] * 16) == capi.RF_ERR_INVALID_ARG and L.rf_last_error_string()


# ---- the refusals of a call, on addresses that are only numbers -----------------------------------------------------------------
SPAN = (2 * 4112 + 4100) * 4      # 3 lines of 4100 samples, 4112 apart
A = [(i + 1) << 20 for i in range(14)]
INVALID = capi.RF_ERR_INVALID_ARG


def raw_call(name, *addresses):
    with host_plan(4100, 3, True, 4112) as plan:
        status = getattr(capi.lib(), name)(plan._h, *(ctypes.c_void_p(a) for a in addresses), None)
        return status, capi.lib().rf_last_error_string().decode()


def put(base, **at):
    """`base` with the addresses at some indices replaced"""
    out = list(base)
    for i, v in at.items():
        out[int(i[1:])] = v
    return out


E = A[:7]      # in, b0, b1, b2, a1, a2, out


@pytest.mark.parametrize("what,addresses,status,text", [
    ("valid: only the host-only refusal is left", E, capi.RF_ERR_HIP, "host-only"),
    *[(f"null pointer {i}", put(E, **{f"i{i}": 0}), INVALID, "null") for i in range(7)],
    ("in 4 bytes off", put(E, i0=A[0] + 4), INVALID, "aligned"),
    ("b2 8 bytes off", put(E, i3=A[3] + 8), INVALID, "aligned"),
    ("out 4 bytes off", put(E, i6=A[6] + 4), INVALID, "aligned"),
    *[(f"out is coefficient {i}", put(E, i6=A[1 + i]), INVALID, f"overlaps coefficient plane {i}") for i in range(5)],
    ("out reaches into a2", put(E, i6=A[5] - SPAN + 16), INVALID, "overlaps coefficient plane 4"),
    ("in == out", put(E, i6=A[0]), INVALID, "in == out is not allowed"),
    ("out overlaps in", put(E, i6=A[0] + 16), INVALID, "overlaps in"),
    # the stated order: null before alignment before the overlaps; a coefficient before in
    ("null before alignment", put(E, i0=A[0] + 4, i5=0), INVALID, "null"),
    ("alignment before overlap", put(E, i1=A[1] + 4, i6=A[0]), INVALID, "aligned"),
    ("a coefficient before in", put(E, i0=A[1], i6=A[1]), INVALID, "overlaps coefficient"),
])
def test_execute_biquad_refusals(what, addresses, status, text):
    got, message = raw_call("rf_var2_plan_execute_biquad", *addresses)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"
    if "in == out" in what:
        assert "neighbouring groups still read in" in message


B = A[:14]     # in, b0, b1, b2, a1, a2, out, grad_out, grad_in, grad_b0, grad_b1, grad_b2, grad_a1, grad_a2
NO_COEF = put(B, i9=0, i10=0, i11=0, i12=0, i13=0)


@pytest.mark.parametrize("what,addresses,status,text", [
    ("valid, with coefficient gradients", B, capi.RF_ERR_HIP, "host-only"),
    ("valid, no coefficient gradients, no out", put(NO_COEF, i6=0), capi.RF_ERR_HIP, "host-only"),
    ("grad_in is grad_out", put(B, i8=A[7]), capi.RF_ERR_HIP, "host-only"),
    *[(f"coefficient gradient {i} alone missing", put(B, **{f"i{9 + i}": 0}), INVALID, "all given or all null") for i in range(5)],
    *[(f"coefficient gradient {i} alone given", put(NO_COEF, **{f"i{9 + i}": A[9 + i]}), INVALID, "all given or all null") for i in range(5)],
    *[(f"null pointer {i}", put(B, **{f"i{i}": 0}), INVALID, "null") for i in (0, 1, 2, 3, 4, 5, 7, 8)],
    ("coefficient gradients without out", put(B, i6=0), INVALID, "null"),
    ("null in without coefficient gradients", put(NO_COEF, i0=0), INVALID, "null"),
    ("grad_a2 4 bytes off", put(B, i13=A[13] + 4), INVALID, "aligned"),
    ("grad_in is b0", put(B, i8=A[1]), INVALID, "grad_in plane 0 overlaps coefficient plane 0"),
    ("grad_in is a2", put(B, i8=A[5]), INVALID, "grad_in plane 0 overlaps coefficient plane 4"),
    ("grad_in is in", put(B, i8=A[0]), INVALID, "grad_in plane 0 overlaps in"),
    ("grad_in is out", put(B, i8=A[6]), INVALID, "grad_in plane 0 overlaps out"),
    ("grad_in overlaps grad_out without being it", put(B, i8=A[7] + 16), INVALID, "overlaps grad_out"),
    ("grad_b1 is in", put(B, i10=A[0]), INVALID, "gradient of coefficient plane 1 overlaps in"),
    ("grad_a1 is out", put(B, i12=A[6]), INVALID, "overlaps out"),
    ("grad_b0 is grad_out", put(B, i9=A[7]), INVALID, "overlaps grad_out"),
    ("grad_b2 is grad_b0", put(B, i11=A[9]), INVALID, "overlaps gradient of coefficient"),
    ("grad_a2 is grad_in", put(B, i13=A[8]), INVALID, "overlaps gradient of coefficient"),
    # the stated order: the mix before a null pointer before alignment before the overlaps
    ("the mix first", put(B, i0=0, i9=0), INVALID, "all given or all null"),
    ("null before alignment", put(B, i1=0, i8=A[8] + 4), INVALID, "null"),
    ("alignment before overlap", put(B, i2=A[2] + 8, i8=A[0]), INVALID, "aligned"),
])
def test_backward_biquad_refusals(what, addresses, status, text):
    got, message = raw_call("rf_var2_plan_backward_biquad", *addresses)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"
