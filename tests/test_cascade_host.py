"""CPU tests of cascades of time-varying direct-form-I sections (rf_var2_plan_execute_cascade / _backward_cascade): the loops of
tests/cascade_loops.py pinned against central differences, the numpy replay of the kernels (tests/cascade_emulator.py) held to
HALF the GPU tests' bar on every case the GPU tests use (the kernels then have a factor of two over the algebra), the exact
identities of the operator in the replay, the exported symbols, the queries, and every refusal of a call in its documented order
on a host-only plan.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest

import biquad_emulator
import cascade_cases as cases
import cascade_emulator as emu
import cascade_loops as loops
import var2_exact as exact
import recfilter_amd as rfa
from recfilter_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = cases.DIRECTIONS
NEW_SYMBOLS = ["rf_var2_plan_execute_cascade", "rf_var2_plan_execute_cascade_timed", "rf_var2_plan_backward_cascade",
               "rf_var2_plan_backward_cascade_timed", "rf_var2_plan_cascade_num_kernels", "rf_var2_plan_backward_cascade_num_kernels",
               "rf_var2_plan_backward_cascade_bytes"]


def name_of(causal):
    return "causal" if causal else "anticausal"


def host_plan(length, lines=1, causal=True, stride=None):
    return rfa.Var2Plan(length, lines=lines, causal=causal, device=capi.RF_DEVICE_HOST_ONLY, stride=stride)


def line(sections, l=0):
    return [tuple(c[l] for c in s) for s in sections]


# ---- the loops ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
def test_adjoint_loops_against_central_differences(causal):
    """the directional derivative of L = sum(g * y) along random directions in x and in one coefficient signal of the first, a
    middle and the last section, f64"""
    n, K, h = 68, 3, 1e-6
    rng = np.random.default_rng(368 + causal)
    x, g = (rng.random((2, n)) * 2 - 1 for _ in range(2))
    sections = []
    for k in range(K):
        a1, a2 = cases.var2_cases.coefficients("resonator", (2, n), rng)
        sections.append([np.asarray(c, dtype=np.float64) for c in (*cases.biquad_cases.taps((2, n), rng), a1, a2)])

    def loss(x, sections):
        return float(np.sum(g * loops.forward(x, sections, causal)[-1]))
    ys = loops.forward(x, sections, causal)
    gx, grads = loops.adjoint(x, sections, ys, g, causal)
    d = rng.random((2, n)) * 2 - 1
    assert abs((loss(x + h * d, sections) - loss(x - h * d, sections)) / (2 * h) - float(np.sum(gx * d))) < 1e-6
    for k, c in [(0, 4), (0, 1), (1, 3), (1, 0), (2, 2), (2, 4)]:
        d = rng.random((2, n)) * 2 - 1
        up, down = [list(s) for s in sections], [list(s) for s in sections]
        up[k][c], down[k][c] = sections[k][c] + h * d, sections[k][c] - h * d
        want = (loss(x, up) - loss(x, down)) / (2 * h)
        assert abs(want - float(np.sum(grads[k][c] * d))) < 1e-6, f"section {k}, {cases.COEFFICIENTS[c]}"
        assert np.any(grads[k][c] != 0)


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_segmented_loops_are_the_loops(causal):
    x, sections, g = cases.case(8196, 1, "sprinkled", causal, 2)
    ys = loops.forward(x, sections, causal)
    gx, grads = loops.adjoint(x, sections, ys, g, causal)
    one = line(sections)
    ys1 = loops.forward(x[0], one, causal, np.float64, True)
    np.testing.assert_allclose(ys1[-1], ys[-1][0], rtol=0, atol=1e-12)
    gx1, grads1 = loops.adjoint(x[0], one, ys1, g[0], causal, np.float64, True)
    for got, want in zip(cases.flat(ys1[-1], (gx1, grads1)), cases.flat(ys[-1], (gx, grads))):
        np.testing.assert_allclose(got, want[0], rtol=0, atol=1e-10)


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [5, 4101])
def test_padding_rule_of_biquad_cascade(n, causal):
    """zeros in every signal behind the end of causal sections, before the start of anticausal ones: the real samples and their
    gradients are the unpadded cascade's"""
    rng = np.random.default_rng(n)
    x, g = (rng.random(n) * 2 - 1 for _ in range(2))
    sections = []
    for _ in range(3):
        a1, a2 = cases.var2_cases.coefficients("resonator", (n,), rng)
        sections.append([np.asarray(c, dtype=np.float64) for c in (*cases.biquad_cases.taps((n,), rng), a1, a2)])
    pad = -n % 4
    where = (0, pad) if causal else (pad, 0)
    keep = np.s_[:n] if causal else np.s_[pad:]
    padded = [[np.pad(c, where) for c in s] for s in sections]
    ys = loops.forward(x, sections, causal)
    pys = loops.forward(np.pad(x, where), padded, causal)
    np.testing.assert_array_equal(pys[-1][keep], ys[-1])
    got = cases.flat(pys[-1], loops.adjoint(np.pad(x, where), padded, pys, np.pad(g, where), causal))
    for a, b in zip(got, cases.flat(ys[-1], loops.adjoint(x, sections, ys, g, causal))):
        np.testing.assert_array_equal(a[keep], b)


# ---- the numpy replay -----------------------------------------------------------------------------------------------------------
def replay(n, lines, kind, causal, K):
    return replay_of(*cases.case(n, lines, kind, causal, K), causal)


def replay_of(x, sections, g, causal):
    (lines, n), K = x.shape, len(sections)
    got = {name: np.empty((lines, n), np.float32) for name in cases.names(K)}
    for l in range(lines):
        one = line(sections, l)
        y = emu.tiled_forward(x[l], one, causal)
        for name, r in zip(cases.names(K), cases.flat(y, emu.tiled_adjoint(x[l], one, y, g[l], causal))):
            got[name][l] = r
    return got


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n,lines,kind,K", cases.GPU_CASES + cases.LONG_MEMORY_CASES)
def test_replay_meets_the_condition_on_every_gpu_case(n, lines, kind, K, causal):
    """forward and all 1 + 5 K gradients of the numpy f32 replay: at most 2 x the f32 serial cascade's error, or under 1e-6"""
    want = cases.expected(n, lines, kind, causal, K)
    got = replay(n, lines, kind, causal, K)
    for name in cases.names(K):
        cases.assert_under_bar(got[name], want[name], f"replay {n} x {lines} {kind} K={K} {name_of(causal)} {name}", factor=2)


def test_every_long_memory_case_has_its_seed():
    assert set(cases.LONG_MEMORY_SEEDS) == {(n, kind, c, K) for n, _, kind, K in cases.LONG_MEMORY_CASES for c in DIRECTIONS}


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", exact.LENGTHS[:2])
def test_replay_is_exact_on_every_exact_gpu_case(n, causal):
    """a section of period 6 into one of period 3, integer taps (tests/var2_exact.py; the closed form is pinned against the loops
    in tests/test_var2_host.py): the replay, the link included, gives the integers -- forward and all 11 gradients"""
    want, left_out = exact.cascade_expected(n, causal)
    assert not left_out and tuple(sorted(want)) == tuple(sorted(cases.names(2)))
    got = replay_of(*exact.cascade_case(n, causal), causal)
    for name in cases.names(2):
        np.testing.assert_array_equal(got[name], want[name], name)


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_a_nan_in_a_masked_slot_reaches_nothing(causal):
    x, sections, g = cases.case(68, 1, "resonator", causal, 4)
    assert all([int(np.isnan(c).sum()) for c in s] == [0, 1, 2, 1, 2] for s in sections)
    assert not any(np.isnan(r).any() for r in replay(68, 1, "resonator", causal, 4).values())


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [64, 68, 4096, 4100, 8196])
def test_zero_feedback_replay_is_successive_sections_in_bits(n, causal):
    """all a = 0: the maps reproduce the samples exactly, so the link's entering state IS the neighbouring tile's samples and
    the cascade is K separate sections bit for bit -- the identity that pins the neighbour rule at tile and group edges"""
    x, sections, _ = cases.case(n, 1, "resonator", causal, 4)
    zero = np.zeros(n, np.float32)
    one = [(b0, b1, b2, zero, zero) for b0, b1, b2, _, _ in line(sections)]
    want = x[0]
    for s in one:
        want = biquad_emulator.tiled_forward(want, *s, causal)
    np.testing.assert_array_equal(emu.tiled_forward(x[0], one, causal).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_one_section_and_identity_sections_in_the_replay(causal):
    n = 4100
    x, sections, _ = cases.case(n, 1, "resonator", causal, 2)
    one = line(sections)
    unit = (np.ones(n, np.float32), *[np.zeros(n, np.float32)] * 4)
    want = emu.tiled_forward(x[0], one, causal)
    np.testing.assert_array_equal(emu.tiled_forward(x[0], one[:1], causal), biquad_emulator.tiled_forward(x[0], *one[0], causal))
    np.testing.assert_array_equal(emu.tiled_forward(x[0], one + [unit, unit], causal), want)
    np.testing.assert_array_equal(emu.tiled_forward(x[0], [unit] + one, causal), want)


# ---- symbols and queries --------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_typed():
    header = open(os.path.join(ROOT, "include", "recfilter_amd.h")).read()
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTED_SYMBOLS
        assert re.search(r"\b" + name + r"\(", header), f"{name} is not declared in recfilter_amd.h"
        assert getattr(L, name).argtypes is not None, f"{name} has no argument types"
    assert L.rf_var2_plan_backward_cascade_bytes.restype is ctypes.c_size_t
    assert len(L.rf_var2_plan_execute_cascade.argtypes) == 6 and len(L.rf_var2_plan_backward_cascade.argtypes) == 9
    assert "#define RF_VAR2_MAX_SECTIONS 16" in header and capi.RF_VAR2_MAX_SECTIONS == 16
    assert ctypes.sizeof(capi.Var2Section) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert capi.RF_ABI == 3 and b"abi 3" in L.rf_version()
    assert "biquad_cascade" in rfa.__all__ and callable(rfa.biquad_cascade)
    for method in ("execute_cascade", "execute_cascade_timed", "backward_cascade", "backward_cascade_timed", "apply_cascade",
                   "cascade_num_kernels", "backward_cascade_num_kernels", "backward_cascade_bytes"):
        assert callable(getattr(rfa.Var2Plan, method))


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("length,lines,stride", [(4, 1, 4), (4096, 1, 4096), (4100, 3, 4112), (1 << 30, 1, 1 << 30)])
def test_queries_of_host_only_plans(length, lines, stride, causal):
    tiles = -(-length // 64)
    groups = -(-tiles // 64)
    span = 4 * ((lines - 1) * stride + length)
    with host_plan(length, lines, causal, stride) as plan:
        for K in range(1, 17):
            assert plan.cascade_num_kernels(K) == 2 * K + 1
            assert plan.backward_cascade_num_kernels(K) == (4 if K == 1 else 6 * K - 1)
            assert plan.backward_cascade_bytes(K) == (span if K == 1 else (K + 1) * span)
        for K in (0, 17, -1):
            assert plan.cascade_num_kernels(K) == 0 and plan.backward_cascade_num_kernels(K) == 0 and plan.backward_cascade_bytes(K) == 0
        assert plan.cascade_num_kernels(1) == plan.biquad_num_kernels
        assert plan.backward_cascade_num_kernels(1) == plan.backward_biquad_num_kernels
        assert plan.backward_cascade_bytes(1) == plan.backward_biquad_bytes
        assert plan.workspace_bytes == 4 * lines * (6 * (tiles + groups) + 2 * groups)      # unchanged
    null = ctypes.c_void_p()
    L = capi.lib()
    assert L.rf_var2_plan_cascade_num_kernels(null, 2) == 0 and L.rf_var2_plan_backward_cascade_num_kernels(null, 2) == 0
    assert L.rf_var2_plan_backward_cascade_bytes(null, 2) == 0


def test_host_only_plan_refuses_to_run_and_a_short_report_is_refused_first():
    sections = [(None,) * 5] * 3
    with host_plan(4096) as plan:
        for call in (lambda: plan.execute_cascade(None, sections), lambda: plan.execute_cascade_timed(None, sections),
                     lambda: plan.backward_cascade(None, sections, None, None), lambda: plan.backward_cascade_timed(None, sections, None, None)):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == capi.RF_ERR_HIP and "host-only" in str(e.value)
        null, ms = ctypes.c_void_p(), (ctypes.c_float * 32)()
        L = capi.lib()
        array = (capi.Var2Section * 3)()
        assert L.rf_var2_plan_execute_cascade_timed(plan._h, null, array, 3, null, null, ms, None, 6) == capi.RF_ERR_INVALID_ARG
        assert b"ms_out too small: need 7" in L.rf_last_error_string()
        assert L.rf_var2_plan_backward_cascade_timed(plan._h, null, array, 3, null, null, null, None, null, ms, None, 16) == capi.RF_ERR_INVALID_ARG
        assert b"ms_out too small: need 17" in L.rf_last_error_string()
        # the names of the launches come back before the first pointer is looked at
        names = (ctypes.c_char_p * 32)()
        assert L.rf_var2_plan_execute_cascade_timed(plan._h, null, array, 3, null, null, ms, names, 32) == capi.RF_ERR_INVALID_ARG
        assert [n.decode() for n in names[:7]] == ["var2_biquad_tails_1d", "var2_carry_1d", "var2_link_1d", "var2_carry_1d", "var2_link_1d",
                                                   "var2_carry_1d", "var2_pass2_1d"]
        assert L.rf_var2_plan_backward_cascade_timed(plan._h, null, array, 3, null, null, null, None, null, ms, names, 32) == capi.RF_ERR_INVALID_ARG
        section = ["var2_adj_tails_1d", "var2_carry_1d", "var2_adj_pass2_1d", "var2_biquad_grad_1d"]
        assert [n.decode() for n in names[:17]] == ["var2_biquad_tails_1d", "var2_carry_1d", "var2_link_keep_1d", "var2_carry_1d",
                                                    "var2_pass2_1d"] + section * 3
        assert L.rf_var2_plan_backward_cascade_timed(plan._h, null, array, 1, null, null, null, None, null, ms, names, 32) == capi.RF_ERR_INVALID_ARG
        assert [n.decode() for n in names[:4]] == section
    assert L.rf_var2_plan_execute_cascade(null, null, None, 1, null, null) == capi.RF_ERR_INVALID_ARG and L.rf_last_error_string()
    assert L.rf_var2_plan_backward_cascade(null, null, None, 1, null, null, null, None, null) == capi.RF_ERR_INVALID_ARG and L.rf_last_error_string()


# ---- the refusals of a call, on addresses that are only numbers -----------------------------------------------------------------
SPAN = (2 * 4112 + 4100) * 4      # 3 lines of 4100 samples, 4112 apart
INVALID = capi.RF_ERR_INVALID_ARG
K = 3
IN, OUT, GOUT, GIN = ((i + 1) << 20 for i in range(4))
COEF = [[(8 + 5 * k + c) << 20 for c in range(5)] for k in range(K)]          # section k: b0, b1, b2, a1, a2
GRAD = [[(40 + 5 * k + c) << 20 for c in range(5)] for k in range(K)]


def sections_of(table, n=K):
    array = (capi.Var2Section * max(n, 1))()
    for k in range(min(n, len(table))):
        for name, address in zip(cases.COEFFICIENTS, table[k]):
            setattr(array[k], name, address or None)
    return array


def changed(table, k, c, value):
    out = [list(s) for s in table]
    out[k][c] = value
    return out


def execute(inp=IN, out=OUT, coef=COEF, n=K, null_sections=False):
    with host_plan(4100, 3, True, 4112) as plan:
        p = ctypes.c_void_p
        status = capi.lib().rf_var2_plan_execute_cascade(plan._h, p(inp), None if null_sections else sections_of(coef, n), n, p(out), None)
        return status, capi.lib().rf_last_error_string().decode()


def backward(inp=IN, out=OUT, gout=GOUT, gin=GIN, coef=COEF, grad=GRAD, n=K, null_sections=False):
    with host_plan(4100, 3, True, 4112) as plan:
        p = ctypes.c_void_p
        status = capi.lib().rf_var2_plan_backward_cascade(plan._h, p(inp), None if null_sections else sections_of(coef, n), n, p(out), p(gout),
                                                          p(gin), None if grad is None else sections_of(grad, n), None)
        return status, capi.lib().rf_last_error_string().decode()


@pytest.mark.parametrize("what,arguments,status,text", [
    ("valid: only the host-only refusal is left", {}, capi.RF_ERR_HIP, "host-only"),
    ("one section", {"n": 1}, capi.RF_ERR_HIP, "host-only"),
    ("no section", {"n": 0}, INVALID, "n_sections must be 1..16 (got 0)"),
    ("17 sections", {"n": 17}, INVALID, "n_sections must be 1..16 (got 17)"),
    ("null sections", {"null_sections": True}, INVALID, "null sections"),
    ("null in", {"inp": 0}, INVALID, "signal 0: null"),
    ("null out", {"out": 0}, INVALID, "signal 0: null"),
    ("in 4 bytes off", {"inp": IN + 4}, INVALID, "signal 0: the var2 scans need 16-byte aligned"),
    ("out 8 bytes off", {"out": OUT + 8}, INVALID, "signal 0: the var2 scans need 16-byte aligned"),
    *[(f"null coefficient {c} of section {k}", {"coef": changed(COEF, k, c, 0)}, INVALID, f"section {k}: null pointer")
      for k in range(K) for c in range(5)],
    *[(f"coefficient {c} of section {k} 4 bytes off", {"coef": changed(COEF, k, c, COEF[k][c] + 4)}, INVALID, f"section {k}: the var2 scans need 16-byte")
      for k, c in [(0, 0), (1, 2), (2, 4)]],
    *[(f"out is coefficient {c} of section {k}", {"out": COEF[k][c]}, INVALID, f"out plane 0 overlaps coefficient of section {k} plane {c}: a coefficient signal is read")
      for k in range(K) for c in range(5)],
    ("out reaches into a2 of section 1", {"out": COEF[1][4] - SPAN + 16}, INVALID, "overlaps coefficient of section 1 plane 4"),
    ("in == out", {"out": IN}, INVALID, "in == out is not allowed"),
    ("out overlaps in", {"out": IN + 16}, INVALID, "out plane 0 overlaps in"),
    # the stated order
    ("the count before null sections", {"n": 0, "null_sections": True}, INVALID, "n_sections"),
    ("null sections before a null signal", {"null_sections": True, "inp": 0}, INVALID, "null sections"),
    ("the signals before the sections", {"out": OUT + 4, "coef": changed(COEF, 0, 0, 0)}, INVALID, "signal 0"),
    ("a section's null before the next one's alignment", {"coef": changed(changed(COEF, 2, 1, COEF[2][1] + 4), 1, 3, 0)}, INVALID, "section 1: null"),
    ("alignment before overlap", {"coef": changed(COEF, 2, 0, COEF[2][0] + 4), "out": IN}, INVALID, "section 2: the var2 scans need"),
    ("a coefficient before in", {"inp": COEF[2][1], "out": COEF[2][1]}, INVALID, "overlaps coefficient of section 2 plane 1"),
])
def test_execute_cascade_refusals(what, arguments, status, text):
    got, message = execute(**arguments)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"
    if "in == out" in what:
        assert "neighbouring groups still read in" in message


@pytest.mark.parametrize("what,arguments,status,text", [
    ("valid, with coefficient gradients", {}, capi.RF_ERR_HIP, "host-only"),
    ("valid, no coefficient gradients, no out", {"grad": None, "out": 0}, capi.RF_ERR_HIP, "host-only"),
    ("grad_in is grad_out", {"gin": GOUT}, capi.RF_ERR_HIP, "host-only"),
    ("no section", {"n": 0}, INVALID, "n_sections must be 1..16 (got 0)"),
    ("17 sections", {"n": 17}, INVALID, "n_sections must be 1..16 (got 17)"),
    ("null sections", {"null_sections": True}, INVALID, "null sections"),
    *[(f"gradient {c} of section {k} alone missing", {"grad": changed(GRAD, k, c, 0)}, INVALID, f"section {k}: the five coefficient gradients are all given")
      for k in range(K) for c in range(5)],
    ("a section without gradients", {"grad": [GRAD[0], [0] * 5, GRAD[2]]}, INVALID, "section 1: the five coefficient gradients are all given, or grads is null (0 given)"),
    *[(f"null {name}", {name: 0}, INVALID, "signal 0: null") for name in ("inp", "gout", "gin")],
    ("coefficient gradients without out", {"out": 0}, INVALID, "signal 0: null"),
    ("grad_in 4 bytes off", {"gin": GIN + 4}, INVALID, "signal 0: the var2 scans need"),
    ("null a1 of section 2", {"coef": changed(COEF, 2, 3, 0)}, INVALID, "section 2: null pointer"),
    ("b1 of section 1 8 bytes off", {"coef": changed(COEF, 1, 1, COEF[1][1] + 8)}, INVALID, "section 1: the var2 scans need"),
    ("grad_a2 of section 2 4 bytes off", {"grad": changed(GRAD, 2, 4, GRAD[2][4] + 4)}, INVALID, "section 2: the var2 scans need 16-byte aligned pointers (a coefficient gradient)"),
    ("grad_in is b0 of section 1", {"gin": COEF[1][0]}, INVALID, "grad_in plane 0 overlaps coefficient of section 1 plane 0"),
    ("grad_in is in", {"gin": IN}, INVALID, "grad_in plane 0 overlaps in"),
    ("grad_in is out", {"gin": OUT}, INVALID, "grad_in plane 0 overlaps out"),
    ("grad_in overlaps grad_out without being it", {"gin": GOUT + 16}, INVALID, "overlaps grad_out"),
    ("grad_b1 of section 2 is in", {"grad": changed(GRAD, 2, 1, IN)}, INVALID, "gradient of section 2 plane 1 overlaps in"),
    ("grad_a1 of section 0 is out", {"grad": changed(GRAD, 0, 3, OUT)}, INVALID, "gradient of section 0 plane 3 overlaps out"),
    ("grad_b0 of section 1 is grad_out", {"grad": changed(GRAD, 1, 0, GOUT)}, INVALID, "gradient of section 1 plane 0 overlaps grad_out"),
    ("grad_b2 of section 0 is a2 of section 2", {"grad": changed(GRAD, 0, 2, COEF[2][4])}, INVALID, "gradient of section 0 plane 2 overlaps coefficient of section 2 plane 4"),
    ("grad_b2 of section 2 is grad_b0 of section 0", {"grad": changed(GRAD, 2, 2, GRAD[0][0])}, INVALID, "gradient of section 0 plane 0 overlaps gradient of section 2 plane 2"),
    ("grad_a2 of section 1 is grad_in", {"grad": changed(GRAD, 1, 4, GIN)}, INVALID, "grad_in plane 0 overlaps gradient of section 1 plane 4"),
    # the stated order
    ("the count first", {"n": 17, "null_sections": True}, INVALID, "n_sections"),
    ("null sections before the mix", {"null_sections": True, "grad": changed(GRAD, 0, 0, 0)}, INVALID, "null sections"),
    ("the mix before a null signal", {"inp": 0, "grad": changed(GRAD, 1, 2, 0)}, INVALID, "section 1: the five"),
    ("a null signal before a section", {"gout": 0, "coef": changed(COEF, 0, 0, COEF[0][0] + 4)}, INVALID, "signal 0: null"),
    ("the coefficients before the gradients' alignment", {"coef": changed(COEF, 2, 0, 0), "grad": changed(GRAD, 0, 0, GRAD[0][0] + 4)}, INVALID, "section 2: null pointer"),
    ("alignment before overlap", {"grad": changed(GRAD, 0, 0, GRAD[0][0] + 4), "gin": IN}, INVALID, "a coefficient gradient"),
])
def test_backward_cascade_refusals(what, arguments, status, text):
    got, message = backward(**arguments)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"
