"""CPU tests of the cascade for training (rf_var2_plan_execute_cascade_keep / _backward_cascade_kept): the numpy replay of the new
backward (tests/cascade_kept_emulator.py) held to HALF the GPU tests' bar on every case the GPU tests use, its exact identities
-- all feedback 0 gives the bits of the rerunning backward's replay, one section is the section's replay -- the exported symbols,
the queries, and every refusal of the two calls in their documented order on a host-only plan.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest

import biquad_emulator
import cascade_cases as cases
import cascade_emulator
import cascade_kept_emulator as emu
import var2_exact as exact
import recfilter_amd as rfa
from recfilter_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = cases.DIRECTIONS
NEW_SYMBOLS = ["rf_var2_plan_execute_cascade_keep", "rf_var2_plan_execute_cascade_keep_timed", "rf_var2_plan_backward_cascade_kept",
               "rf_var2_plan_backward_cascade_kept_timed", "rf_var2_plan_backward_cascade_kept_num_kernels",
               "rf_var2_plan_backward_cascade_kept_bytes"]


def name_of(causal):
    return "causal" if causal else "anticausal"


def host_plan(length, lines=1, causal=True, stride=None):
    return rfa.Var2Plan(length, lines=lines, causal=causal, device=capi.RF_DEVICE_HOST_ONLY, stride=stride)


def line(sections, l=0):
    return [tuple(c[l] for c in s) for s in sections]


# ---- the numpy replay -----------------------------------------------------------------------------------------------------------
def replay_of(x, sections, g, causal):
    """{name: (lines, n)} of the gradients, names cascade_cases.names(K)[1:]"""
    (lines, n), K = x.shape, len(sections)
    got = {name: np.empty((lines, n), np.float32) for name in cases.names(K)[1:]}
    for l in range(lines):
        one, results = line(sections, l), []
        cascade_emulator.tiled_forward(x[l], one, causal, results)
        gx, grads = emu.tiled_adjoint(x[l], one, results, g[l], causal)
        for name, r in zip(cases.names(K)[1:], [gx] + [c for s in grads for c in s]):
            got[name][l] = r
    return got


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n,lines,kind,K", [c for c in cases.GPU_CASES + cases.LONG_MEMORY_CASES if c[0] < cases.LONG])
def test_replay_meets_the_condition_on_every_gpu_case(n, lines, kind, K, causal):
    """all 1 + 5 K gradients of the numpy f32 replay: at most 2 x the f32 serial cascade's error, or under 1e-6"""
    want = cases.expected(n, lines, kind, causal, K)
    got = replay_of(*cases.case(n, lines, kind, causal, K), causal)
    for name in cases.names(K)[1:]:
        cases.assert_under_bar(got[name], want[name], f"kept replay {n} x {lines} {kind} K={K} {name_of(causal)} {name}", factor=2)


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [64, 68, 4096, 4100, 8196])
def test_zero_feedback_replay_is_the_rerunning_backward_in_bits(n, causal):
    """all a = 0: the maps reproduce the samples exactly, so the adjoint link's entering state IS the neighbouring tile's lam and
    the new backward is the old one bit for bit -- the identity that pins the neighbour rule at tile and group edges"""
    x, sections, g = cases.case(n, 1, "resonator", causal, 4)
    zero = np.zeros(n, np.float32)
    one = [(b0, b1, b2, zero, zero) for b0, b1, b2, _, _ in line(sections)]
    results = []
    y = cascade_emulator.tiled_forward(x[0], one, causal, results)
    want_x, want = cascade_emulator.tiled_adjoint(x[0], one, y, g[0], causal)
    got_x, got = emu.tiled_adjoint(x[0], one, results, g[0], causal)
    np.testing.assert_array_equal(got_x.view(np.uint32), want_x.view(np.uint32))
    for k in range(4):
        for c in range(5):
            np.testing.assert_array_equal(got[k][c].view(np.uint32), want[k][c].view(np.uint32), f"section {k} {cases.COEFFICIENTS[c]}")


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_one_section_is_the_sections_replay_in_bits(causal):
    x, sections, g = cases.case(4100, 1, "resonator", causal, 1)
    one = line(sections)
    y = biquad_emulator.tiled_forward(x[0], *one[0], causal)
    want = biquad_emulator.tiled_adjoint(x[0], *one[0], y, g[0], causal)
    gx, grads = emu.tiled_adjoint(x[0], one, [y], g[0], causal)
    for got, ref in zip([gx, *grads[0]], want):
        np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_a_nan_in_a_masked_slot_reaches_nothing(causal):
    x, sections, g = cases.case(68, 1, "resonator", causal, 4)
    assert all([int(np.isnan(c).sum()) for c in s] == [0, 1, 2, 1, 2] for s in sections)
    assert not any(np.isnan(r).any() for r in replay_of(x, sections, g, causal).values())


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_replay_is_exact_on_the_exact_gpu_case(causal):
    """integer sections of periods 6 and 3 at four groups: the replay, the adjoint link included, gives the integers"""
    n = exact.LENGTHS[0]
    want, left_out = exact.cascade_expected(n, causal)
    assert not left_out
    got = replay_of(*exact.cascade_case(n, causal), causal)
    for name in cases.names(2)[1:]:
        np.testing.assert_array_equal(got[name], want[name], name)


# ---- symbols and queries --------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_typed():
    header = open(os.path.join(ROOT, "include", "recfilter_amd.h")).read()
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTED_SYMBOLS
        assert re.search(r"\b" + name + r"\(", header), f"{name} is not declared in recfilter_amd.h"
        assert getattr(L, name).argtypes is not None, f"{name} has no argument types"
    assert L.rf_var2_plan_backward_cascade_kept_bytes.restype is ctypes.c_size_t
    assert len(L.rf_var2_plan_execute_cascade_keep.argtypes) == 7 and len(L.rf_var2_plan_backward_cascade_kept.argtypes) == 10
    assert len(L.rf_var2_plan_execute_cascade_keep_timed.argtypes) == 10 and len(L.rf_var2_plan_backward_cascade_kept_timed.argtypes) == 13
    assert capi.RF_ABI == 3 and b"abi 3" in L.rf_version()
    for method in ("execute_cascade_keep", "execute_cascade_keep_timed", "backward_cascade_kept", "backward_cascade_kept_timed",
                   "backward_cascade_kept_num_kernels", "backward_cascade_kept_bytes"):
        assert callable(getattr(rfa.Var2Plan, method))
    for where in (os.path.join("include", "recfilter_amd.h"), "README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, where)).read()
        assert not re.search(r"keeping\s+(the\s+)?forward('s)?\s+intermediates", text, re.I), f"{where} still lists kept intermediates as out of scope"


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("length,lines,stride", [(4, 1, 4), (4096, 1, 4096), (4100, 3, 4112), (1 << 30, 1, 1 << 30)])
def test_queries_of_host_only_plans(length, lines, stride, causal):
    tiles = -(-length // 64)
    groups = -(-tiles // 64)
    span = 4 * ((lines - 1) * stride + length)
    with host_plan(length, lines, causal, stride) as plan:
        for K in range(1, 17):
            assert plan.backward_cascade_kept_num_kernels(K, False) == 2 * K + 2
            assert plan.backward_cascade_kept_num_kernels(K, True) == 3 * K + 1
            assert plan.backward_cascade_kept_bytes(K) == (span if K == 1 else 2 * span)
            # the existing queries keep their values
            assert plan.cascade_num_kernels(K) == 2 * K + 1
            assert plan.backward_cascade_num_kernels(K) == (4 if K == 1 else 6 * K - 1)
            assert plan.backward_cascade_bytes(K) == (span if K == 1 else (K + 1) * span)
        for K in (0, 17, -1):
            assert plan.backward_cascade_kept_num_kernels(K, False) == 0 and plan.backward_cascade_kept_num_kernels(K, True) == 0
            assert plan.backward_cascade_kept_bytes(K) == 0
        assert plan.backward_cascade_kept_num_kernels(1, False) == plan.backward_cascade_kept_num_kernels(1, True) == plan.backward_biquad_num_kernels
        assert plan.backward_cascade_kept_bytes(1) == plan.backward_biquad_bytes
        assert plan.workspace_bytes == 4 * lines * (6 * (tiles + groups) + 2 * groups)      # unchanged
    null = ctypes.c_void_p()
    L = capi.lib()
    assert L.rf_var2_plan_backward_cascade_kept_num_kernels(null, 2, 1) == 0 and L.rf_var2_plan_backward_cascade_kept_bytes(null, 2) == 0


def test_host_only_plan_refuses_to_run_and_a_short_report_is_refused_first():
    sections = [(None,) * 5] * 3
    with host_plan(4096) as plan:
        for call in (lambda: plan.execute_cascade_keep(None, sections), lambda: plan.execute_cascade_keep_timed(None, sections),
                     lambda: plan.backward_cascade_kept(None, sections, None, None, None),
                     lambda: plan.backward_cascade_kept_timed(None, sections, None, None, None)):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == capi.RF_ERR_HIP and "host-only" in str(e.value)
        null, ms = ctypes.c_void_p(), (ctypes.c_float * 64)()
        L = capi.lib()
        array, garray = (capi.Var2Section * 3)(), (capi.Var2Section * 3)()
        assert L.rf_var2_plan_execute_cascade_keep_timed(plan._h, null, array, 3, null, None, null, ms, None, 6) == capi.RF_ERR_INVALID_ARG
        assert b"ms_out too small: need 7" in L.rf_last_error_string()
        assert L.rf_var2_plan_backward_cascade_kept_timed(plan._h, null, array, 3, None, null, null, null, None, null, ms, None, 7) == capi.RF_ERR_INVALID_ARG
        assert b"ms_out too small: need 8" in L.rf_last_error_string()
        assert L.rf_var2_plan_backward_cascade_kept_timed(plan._h, null, array, 3, None, null, null, null, garray, null, ms, None, 9) == capi.RF_ERR_INVALID_ARG
        assert b"ms_out too small: need 10" in L.rf_last_error_string()
        # the names of the launches come back before the first pointer is looked at
        names = (ctypes.c_char_p * 64)()
        assert L.rf_var2_plan_execute_cascade_keep_timed(plan._h, null, array, 3, null, None, null, ms, names, 64) == capi.RF_ERR_INVALID_ARG
        assert [n.decode() for n in names[:7]] == forward_names(3)
        for K in (1, 2, 3, 16):
            for grads in (None, (capi.Var2Section * 16)()):
                assert L.rf_var2_plan_backward_cascade_kept_timed(plan._h, null, (capi.Var2Section * 16)(), K, None, null, null, null, grads, null, ms,
                                                                  names, 64) == capi.RF_ERR_INVALID_ARG
                want = backward_names(K, grads is not None)
                assert [n.decode() for n in names[:len(want)]] == want
    assert L.rf_var2_plan_execute_cascade_keep(null, null, None, 1, null, None, null) == capi.RF_ERR_INVALID_ARG and L.rf_last_error_string()
    assert L.rf_var2_plan_backward_cascade_kept(null, null, None, 1, None, null, null, null, None, null) == capi.RF_ERR_INVALID_ARG and L.rf_last_error_string()


def forward_names(K):
    return ["var2_biquad_tails_1d"] + ["var2_carry_1d", "var2_link_keep_1d"] * (K - 1) + ["var2_carry_1d", "var2_pass2_1d"]


def backward_names(K, with_coefficients):
    link = ["var2_carry_1d", "var2_adj_link_keep_1d", "var2_biquad_coef_1d"] if with_coefficients else ["var2_carry_1d", "var2_adj_link_1d"]
    names = ["var2_adj_tails_1d"] + link * (K - 1) + ["var2_carry_1d", "var2_adj_pass2_1d", "var2_biquad_grad_1d"]
    assert len(names) == (3 * K + 1 if with_coefficients else 2 * K + 2)
    return names


# ---- the refusals of a call, on addresses that are only numbers -----------------------------------------------------------------
SPAN = (2 * 4112 + 4100) * 4      # 3 lines of 4100 samples, 4112 apart
INVALID = capi.RF_ERR_INVALID_ARG
K = 3
IN, OUT, GOUT, GIN = ((i + 1) << 20 for i in range(4))
COEF = [[(8 + 5 * k + c) << 20 for c in range(5)] for k in range(K)]          # section k: b0, b1, b2, a1, a2
GRAD = [[(40 + 5 * k + c) << 20 for c in range(5)] for k in range(K)]
KEPT = [(60 + k) << 20 for k in range(K - 1)]


def sections_of(table, n=K):
    array = (capi.Var2Section * max(n, 1))()
    for k in range(min(n, len(table))):
        for name, address in zip(cases.COEFFICIENTS, table[k]):
            setattr(array[k], name, address or None)
    return array


def kept_of(kept):
    return None if kept is None else (ctypes.c_void_p * max(len(kept), 1))(*(a or None for a in kept))


def changed(table, k, c, value):
    out = [list(s) for s in table]
    out[k][c] = value
    return out


def kept_changed(k, value):
    out = list(KEPT)
    out[k] = value
    return out


def execute(inp=IN, out=OUT, coef=COEF, kept=KEPT, n=K, null_sections=False):
    with host_plan(4100, 3, True, 4112) as plan:
        p = ctypes.c_void_p
        status = capi.lib().rf_var2_plan_execute_cascade_keep(plan._h, p(inp), None if null_sections else sections_of(coef, n), n, p(out),
                                                              kept_of(kept), None)
        return status, capi.lib().rf_last_error_string().decode()


def backward(inp=IN, out=OUT, gout=GOUT, gin=GIN, coef=COEF, grad=GRAD, kept=KEPT, n=K, null_sections=False):
    with host_plan(4100, 3, True, 4112) as plan:
        p = ctypes.c_void_p
        status = capi.lib().rf_var2_plan_backward_cascade_kept(plan._h, p(inp), None if null_sections else sections_of(coef, n), n, kept_of(kept),
                                                               p(out), p(gout), p(gin), None if grad is None else sections_of(grad, n), None)
        return status, capi.lib().rf_last_error_string().decode()


@pytest.mark.parametrize("what,arguments,status,text", [
    ("valid: only the host-only refusal is left", {}, capi.RF_ERR_HIP, "host-only"),
    ("one section, no kept array", {"n": 1, "kept": None}, capi.RF_ERR_HIP, "host-only"),
    ("no section", {"n": 0}, INVALID, "n_sections must be 1..16 (got 0)"),
    ("17 sections", {"n": 17}, INVALID, "n_sections must be 1..16 (got 17)"),
    ("null sections", {"null_sections": True}, INVALID, "null sections"),
    ("null in", {"inp": 0}, INVALID, "signal 0: null"),
    ("null out", {"out": 0}, INVALID, "signal 0: null"),
    ("out 8 bytes off", {"out": OUT + 8}, INVALID, "signal 0: the var2 scans need 16-byte aligned"),
    ("no kept array", {"kept": None}, INVALID, "kept 0: null pointer"),
    ("null kept 0", {"kept": kept_changed(0, 0)}, INVALID, "kept 0: null pointer"),
    ("null kept 1", {"kept": kept_changed(1, 0)}, INVALID, "kept 1: null pointer"),
    ("kept 1 4 bytes off", {"kept": kept_changed(1, KEPT[1] + 4)}, INVALID, "kept 1: the var2 scans need 16-byte aligned"),
    ("null coefficient", {"coef": changed(COEF, 1, 2, 0)}, INVALID, "section 1: null pointer"),
    ("out is a coefficient", {"out": COEF[2][3]}, INVALID, "out plane 0 overlaps coefficient of section 2 plane 3: a coefficient signal is read"),
    ("in == out", {"out": IN}, INVALID, "in == out is not allowed"),
    ("kept 0 is out", {"kept": kept_changed(0, OUT)}, INVALID, "out plane 0 overlaps kept plane 0"),
    ("kept 1 reaches into out", {"kept": kept_changed(1, OUT + SPAN - 16)}, INVALID, "out plane 0 overlaps kept plane 1"),
    ("kept 1 is in", {"kept": kept_changed(1, IN)}, INVALID, "kept plane 1 overlaps in"),
    *[(f"kept 0 is coefficient {c} of section {k}", {"kept": kept_changed(0, COEF[k][c])}, INVALID, f"kept plane 0 overlaps coefficient of section {k} plane {c}")
      for k in range(K) for c in range(5)],
    ("kept 1 is kept 0", {"kept": [KEPT[0], KEPT[0]]}, INVALID, "kept plane 0 overlaps kept plane 1"),
    # the stated order
    ("the count before null sections", {"n": 0, "null_sections": True}, INVALID, "n_sections"),
    ("the signals before the kept pointers", {"out": OUT + 4, "kept": None}, INVALID, "signal 0"),
    ("the kept pointers before the sections", {"kept": kept_changed(1, 0), "coef": changed(COEF, 0, 0, 0)}, INVALID, "kept 1: null"),
    ("alignment before overlap", {"coef": changed(COEF, 2, 0, COEF[2][0] + 4), "kept": kept_changed(0, OUT)}, INVALID, "section 2: the var2 scans need"),
])
def test_execute_cascade_keep_refusals(what, arguments, status, text):
    got, message = execute(**arguments)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"


@pytest.mark.parametrize("what,arguments,status,text", [
    ("valid, with coefficient gradients", {}, capi.RF_ERR_HIP, "host-only"),
    ("valid, no coefficient gradients: nothing of the forward", {"grad": None, "out": 0, "inp": 0, "kept": None}, capi.RF_ERR_HIP, "host-only"),
    ("valid, no coefficient gradients, kept entries null", {"grad": None, "kept": [0, 0]}, capi.RF_ERR_HIP, "host-only"),
    ("one section, no kept array", {"n": 1, "kept": None}, capi.RF_ERR_HIP, "host-only"),
    ("grad_in is grad_out", {"gin": GOUT}, capi.RF_ERR_HIP, "host-only"),
    ("no section", {"n": 0}, INVALID, "n_sections must be 1..16 (got 0)"),
    ("17 sections", {"n": 17}, INVALID, "n_sections must be 1..16 (got 17)"),
    ("null sections", {"null_sections": True}, INVALID, "null sections"),
    *[(f"gradient {c} of section {k} alone missing", {"grad": changed(GRAD, k, c, 0)}, INVALID, f"section {k}: the five coefficient gradients are all given")
      for k, c in [(0, 0), (1, 3), (2, 4)]],
    ("a section without gradients", {"grad": [GRAD[0], [0] * 5, GRAD[2]]}, INVALID, "section 1: the five coefficient gradients are all given, or grads is null (0 given)"),
    *[(f"null {name}", {name: 0}, INVALID, "signal 0: null") for name in ("gout", "gin")],
    ("coefficient gradients without in", {"inp": 0}, INVALID, "signal 0: null"),
    ("coefficient gradients without out", {"out": 0}, INVALID, "signal 0: null"),
    ("coefficient gradients without the kept array", {"kept": None}, INVALID, "kept 0: null pointer"),
    ("coefficient gradients without kept 1", {"kept": kept_changed(1, 0)}, INVALID, "kept 1: null pointer"),
    ("kept 0 8 bytes off", {"kept": kept_changed(0, KEPT[0] + 8)}, INVALID, "kept 0: the var2 scans need 16-byte aligned"),
    ("kept 0 8 bytes off, no coefficient gradients", {"grad": None, "kept": kept_changed(0, KEPT[0] + 8)}, INVALID, "kept 0: the var2 scans need"),
    ("grad_in 4 bytes off", {"gin": GIN + 4}, INVALID, "signal 0: the var2 scans need"),
    ("null a1 of section 2", {"coef": changed(COEF, 2, 3, 0)}, INVALID, "section 2: null pointer"),
    ("grad_a2 of section 2 4 bytes off", {"grad": changed(GRAD, 2, 4, GRAD[2][4] + 4)}, INVALID, "section 2: the var2 scans need 16-byte aligned pointers (a coefficient gradient)"),
    ("grad_in is b0 of section 1", {"gin": COEF[1][0]}, INVALID, "grad_in plane 0 overlaps coefficient of section 1 plane 0"),
    ("grad_in is in", {"gin": IN}, INVALID, "grad_in plane 0 overlaps in"),
    ("grad_in is out", {"gin": OUT}, INVALID, "grad_in plane 0 overlaps out"),
    ("grad_in is kept 1", {"gin": KEPT[1]}, INVALID, "grad_in plane 0 overlaps kept plane 1"),
    ("grad_in overlaps grad_out without being it", {"gin": GOUT + 16}, INVALID, "overlaps grad_out"),
    ("grad_b1 of section 2 is kept 0", {"grad": changed(GRAD, 2, 1, KEPT[0])}, INVALID, "gradient of section 2 plane 1 overlaps kept plane 0"),
    ("grad_a1 of section 0 reaches into kept 1", {"grad": changed(GRAD, 0, 3, KEPT[1] - SPAN + 16)}, INVALID, "gradient of section 0 plane 3 overlaps kept plane 1"),
    ("grad_b0 of section 1 is grad_out", {"grad": changed(GRAD, 1, 0, GOUT)}, INVALID, "gradient of section 1 plane 0 overlaps grad_out"),
    ("grad_b2 of section 0 is a2 of section 2", {"grad": changed(GRAD, 0, 2, COEF[2][4])}, INVALID, "gradient of section 0 plane 2 overlaps coefficient of section 2 plane 4"),
    ("grad_b2 of section 2 is grad_b0 of section 0", {"grad": changed(GRAD, 2, 2, GRAD[0][0])}, INVALID, "gradient of section 0 plane 0 overlaps gradient of section 2 plane 2"),
    # the stated order
    ("the count first", {"n": 17, "null_sections": True}, INVALID, "n_sections"),
    ("the mix before a null signal", {"gout": 0, "grad": changed(GRAD, 1, 2, 0)}, INVALID, "section 1: the five"),
    ("a null signal before the kept pointers", {"gout": 0, "kept": None}, INVALID, "signal 0: null"),
    ("the kept pointers before a section", {"kept": kept_changed(0, 0), "coef": changed(COEF, 0, 0, COEF[0][0] + 4)}, INVALID, "kept 0: null"),
    ("the coefficients before the gradients' alignment", {"coef": changed(COEF, 2, 0, 0), "grad": changed(GRAD, 0, 0, GRAD[0][0] + 4)}, INVALID, "section 2: null pointer"),
    ("alignment before overlap", {"grad": changed(GRAD, 0, 0, GRAD[0][0] + 4), "gin": KEPT[0]}, INVALID, "a coefficient gradient"),
])
def test_backward_cascade_kept_refusals(what, arguments, status, text):
    got, message = backward(**arguments)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"
