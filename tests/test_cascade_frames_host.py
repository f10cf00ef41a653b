"""CPU tests of cascades on control-rate frames (rf_var2_plan_execute_cascade_frames / _backward_cascade_frames): the condition the
seeds of tests/cascade_frames_cases.py are chosen by -- the numpy replay of the kernels at or below half the GPU tests' bar on every
output of every case -- the three carry mutants of tests/test_var2_carry_seen_host.py on the case whose carry matrix reaches the
result through both link kernels, and, on a host-only plan, the launch counts and names, the byte queries and every refusal in the
header's order.  No kernel is launched."""
import ctypes
import functools

import numpy as np
import pytest

import cascade_emulator
import cascade_frames_cases as cases
import cascade_kept_emulator
import frames_loops as loops
import recfilter_amd as rfa
import var2_emulator as emu
from recfilter_amd import capi
from test_var2_carry_seen_host import CLEAN_SCAN, MUTANTS

NEW_SYMBOLS = ["rf_var2_plan_execute_cascade_frames", "rf_var2_plan_execute_cascade_frames_timed", "rf_var2_plan_backward_cascade_frames",
               "rf_var2_plan_backward_cascade_frames_timed", "rf_var2_plan_cascade_frames_num_kernels",
               "rf_var2_plan_backward_cascade_frames_num_kernels", "rf_var2_plan_backward_cascade_frames_bytes"]
INVALID, UNSUPPORTED, HOST_ONLY = capi.RF_ERR_INVALID_ARG, capi.RF_ERR_UNSUPPORTED, capi.RF_ERR_HIP


def name_of(causal):
    return "causal" if causal else "anticausal"


def host_plan(length, lines=1, causal=True, stride=None):
    return rfa.Var2Plan(length, lines=lines, causal=causal, device=capi.RF_DEVICE_HOST_ONLY, stride=stride)


# ---- the seeds ----------------------------------------------------------------------------------------------------------------------
def replay(hop, n, lines, K, kind, causal):
    """{name: array} of the kernels' arithmetic in numpy: the f32 expansion, tests/cascade_emulator.py's forward keeping every
    section's result, tests/cascade_kept_emulator.py's backward on them, the 5 K per-sample gradients contracted in f64 and
    rounded once to f32"""
    x, sections, g = cases.case(hop, n, lines, K, kind, causal)
    count = loops.frames_count(n, hop)
    signals = cases.expand_sections(sections, hop, n, np.float32)
    got = {name: np.empty((lines, n if name in ("out", "grad_x") else count), np.float32) for name in cases.names(K)}
    for l in range(lines):
        one = [tuple(c[l] for c in s) for s in signals]
        results = []
        got["out"][l] = cascade_emulator.tiled_forward(x[l], one, causal, results)
        gx, grads = cascade_kept_emulator.tiled_adjoint(x[l], one, results, g[l], causal)
        got["grad_x"][l] = gx
        for name, p in zip(cases.names(K)[2:], [p for s in grads for p in s]):
            got[name][l] = loops.contract(p, hop, count, np.float64).astype(np.float32)
    return got


@pytest.mark.parametrize("hop,n,lines,K,kind,causal", cases.UNDER_THE_BAR)
def test_replay_at_or_below_half_the_bar_on_every_gpu_case(hop, n, lines, K, kind, causal):
    want = cases.expected(hop, n, lines, K, kind, causal)
    got = replay(hop, n, lines, K, kind, causal)
    for name in cases.names(K):
        cases.assert_under_half_the_bar(got[name], want[name], f"replay hop {hop} {n} x {lines} K={K} {kind} {name_of(causal)} {name}")


def test_the_cases_without_a_seed_are_the_two_the_table_names():
    assert cases.NO_SEED == {(64, 4100, 1, 16, "long memory", True), (64, 4100, 1, 16, "long memory", False)}
    assert len(cases.UNDER_THE_BAR) == len(cases.ALL) - 2 and all(c in cases.ALL for c in cases.NO_SEED)
    assert all(key in cases.ALL and 0 < seed < 32 for key, seed in cases.SEEDS.items())


# ---- would the cases see a wrong carry stage? -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", cases.DIRECTIONS)
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_carry_mutants_are_far_above_the_bar(mutant, causal, monkeypatch):
    """(8192, 12292, 1, 2) long memory: four groups, an interval spans groups.  The replay with a wrong carry stage is at least
    100 x the bar on out and on grad_x"""
    hop, n, lines, K, kind = 8192, 3 * 4096 + 4, 1, 2, "long memory"
    want = cases.expected(hop, n, lines, K, kind, causal)
    monkeypatch.setattr(emu, "tiled_scan", functools.partial(CLEAN_SCAN, **MUTANTS[mutant]))
    got = replay(hop, n, lines, K, kind, causal)
    for name in ("out", "grad_x"):
        reference, err32, peak = want[name]
        err = cases._figure(got[name], reference, peak)
        bar = max(4 * err32, 1e-6)
        print(f"{mutant}, {name_of(causal)} {name}: err/peak {err:.3e}, {err / bar:.0f} x the bar")
        assert err >= 100 * bar or np.isnan(err), f"{mutant} {name}: at {err / bar:.1f} x the bar only"


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_front_end():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTED_SYMBOLS and getattr(L, name)
    assert capi.RF_ABI == 3 and b"abi 3" in L.rf_version()
    assert "biquad_cascade_frames" in rfa.__all__ and callable(rfa.biquad_cascade_frames)
    for method in ("execute_cascade_frames", "execute_cascade_frames_timed", "backward_cascade_frames", "backward_cascade_frames_timed",
                   "apply_cascade_frames", "cascade_frames_num_kernels", "backward_cascade_frames_num_kernels", "backward_cascade_frames_bytes"):
        assert callable(getattr(rfa.Var2Plan, method))


def forward_names(K, keep):
    if K == 1:
        return ["var2_biquad_frames_tails_1d", "var2_carry_1d", "var2_frames_pass2_1d"]
    link = "var2_frames_link_keep_1d" if keep else "var2_frames_link_1d"
    return ["var2_biquad_frames_tails_1d"] + ["var2_carry_1d", link] * (K - 1) + ["var2_carry_1d", "var2_frames_pass2_1d"]


def backward_names(K, with_frames):
    last = ["var2_carry_1d", "var2_adj_frames_pass2_1d", "var2_biquad_frames_grad_1d"]
    if K == 1:
        return ["var2_adj_frames_tails_1d"] + last + (["var2_frames_fold_1d"] if with_frames else [])
    boundary = ["var2_carry_1d", "var2_adj_frames_link_keep_1d", "var2_frames_coef_1d"] if with_frames else ["var2_carry_1d", "var2_adj_frames_link_1d"]
    return ["var2_adj_frames_tails_1d"] + boundary * (K - 1) + last + (["var2_frames_fold_cascade_1d"] if with_frames else [])


def reported_names(call, n):
    """the names a *_timed call reports before a host-only plan refuses to run"""
    ms, names = (ctypes.c_float * n)(), (ctypes.c_char_p * n)()
    assert call(ms, names, n) == HOST_ONLY and b"host-only" in capi.lib().rf_last_error_string()
    return [names[i].decode() for i in range(n)]


@pytest.mark.parametrize("K", [1, 2, 16])
def test_launch_counts_and_names_from_the_timed_calls(K):
    hop, n = 64, 4100
    L = capi.lib()
    with host_plan(n) as plan:
        assert plan.cascade_frames_num_kernels(K) == len(forward_names(K, False)) == (3 if K == 1 else 2 * K + 1)
        assert plan.backward_cascade_frames_num_kernels(K, False) == len(backward_names(K, False)) == (4 if K == 1 else 2 * K + 2)
        assert plan.backward_cascade_frames_num_kernels(K, True) == len(backward_names(K, True)) == (5 if K == 1 else 3 * K + 2)
        sections = [None] * K
        for keep in (False, True):
            *p, _, _, s = plan._cascade_frames_arguments(None, sections, hop, None, keep, None, None)
            got = reported_names(lambda *r: L.rf_var2_plan_execute_cascade_frames_timed(plan._h, *p, s, *r), plan.cascade_frames_num_kernels(K))
            assert got == forward_names(K, keep)
        for with_frames in (False, True):
            *p, _, _, s = plan._backward_cascade_frames_arguments(None, sections, hop, None, None, None, None, [None] * K if with_frames else None, None)
            got = reported_names(lambda *r: L.rf_var2_plan_backward_cascade_frames_timed(plan._h, *p, s, *r),
                                 plan.backward_cascade_frames_num_kernels(K, with_frames))
            assert got == backward_names(K, with_frames)
        # a report one slot short is refused behind the section count and before everything else
        *p, _, _, s = plan._cascade_frames_arguments(None, sections, hop, None, False, None, None)
        short = plan.cascade_frames_num_kernels(K) - 1
        assert L.rf_var2_plan_execute_cascade_frames_timed(plan._h, *p, s, (ctypes.c_float * 64)(), None, short) == INVALID
        assert b"ms_out" in L.rf_last_error_string()


@pytest.mark.parametrize("length,lines,stride", [(4, 1, 4), (4096, 1, 4096), (4100, 3, 4112), (1 << 30, 1, 1 << 30)])
def test_queries_of_host_only_plans(length, lines, stride):
    tiles = -(-length // 64)
    groups = -(-tiles // 64)
    with host_plan(length, lines, True, stride) as plan:
        span = 4 * ((lines - 1) * stride + length)
        for hop in (64, 512, 1024, 4096, 65536):
            slab = 80 * lines * -(-length // min(hop, 1024))
            assert plan.backward_cascade_frames_bytes(1, hop) == span + slab == plan.backward_biquad_frames_bytes(hop)
            for K in (2, 3, 16):
                assert plan.backward_cascade_frames_bytes(K, hop) == 2 * span + K * slab
        for K, hop in ((0, 64), (17, 64), (-1, 64), (2, 480), (2, 32), (2, 131072)):
            assert plan.backward_cascade_frames_bytes(K, hop) == 0
        for K in (0, 17):
            assert plan.cascade_frames_num_kernels(K) == 0 and plan.backward_cascade_frames_num_kernels(K, True) == 0
        assert plan.workspace_bytes == 4 * lines * (6 * (tiles + groups) + 2 * groups)      # unchanged
    null, L = ctypes.c_void_p(), capi.lib()
    assert L.rf_var2_plan_cascade_frames_num_kernels(null, 2) == 0 and L.rf_var2_plan_backward_cascade_frames_num_kernels(null, 2, 1) == 0
    assert L.rf_var2_plan_backward_cascade_frames_bytes(null, 2, 64) == 0


# ---- the refusals of a call, on addresses that are only numbers ---------------------------------------------------------------------
LENGTH, LINES, STRIDE, HOP = 4100, 3, 4112, 64
COUNT = 66                                    # ceil(4100 / 64) + 1
FSTRIDE = COUNT + 2
SPAN = (2 * STRIDE + LENGTH) * 4
K = 3
A = [(i + 1) << 20 for i in range(64)]
X, OUT, GOUT, GIN = A[:4]
KEPT = A[4:6]
FRAMES = [A[8 + 5 * k:13 + 5 * k] for k in range(K)]            # A[8] .. A[22]
GRADS = [A[24 + 5 * k:29 + 5 * k] for k in range(K)]            # A[24] .. A[38]


def sections_of(rows):
    if rows is None:
        return None
    return (capi.Var2Section * len(rows))(*(capi.Var2Section(*r) for r in rows))


def pointers(values):
    return None if values is None else (ctypes.c_void_p * max(len(values), 1))(*values)


def put(base, **at):
    out = dict(base)
    out.update(at)
    return out


def with_row(rows, k, i, value):
    rows = [list(r) for r in rows]
    rows[k][i] = value
    return rows


def raw_forward(a):
    with host_plan(LENGTH, LINES, True, STRIDE) as plan:
        status = capi.lib().rf_var2_plan_execute_cascade_frames(plan._h, ctypes.c_void_p(a["x"]), sections_of(a["frames"]), a["K"], a["hop"], a["count"],
                                                                a["fstride"], ctypes.c_void_p(a["out"]), pointers(a["kept"]), None)
        return status, capi.lib().rf_last_error_string().decode()


def raw_backward(a):
    with host_plan(LENGTH, LINES, True, STRIDE) as plan:
        status = capi.lib().rf_var2_plan_backward_cascade_frames(
            plan._h, ctypes.c_void_p(a["x"]), sections_of(a["frames"]), a["K"], a["hop"], a["count"], a["fstride"], pointers(a["kept"]),
            ctypes.c_void_p(a["out"]), ctypes.c_void_p(a["gout"]), ctypes.c_void_p(a["gin"]), sections_of(a["grads"]), None)
        return status, capi.lib().rf_last_error_string().decode()


E = dict(x=X, frames=FRAMES, K=K, hop=HOP, count=COUNT, fstride=FSTRIDE, out=OUT, kept=None)
EK = put(E, kept=KEPT)


@pytest.mark.parametrize("what,a,status,text", [
    ("valid: only the host-only refusal is left", E, HOST_ONLY, "host-only"),
    ("valid, keeping", EK, HOST_ONLY, "host-only"),
    ("one section is the section's call", put(E, K=1), HOST_ONLY, "host-only"),
    ("sixteen sections", put(E, K=16, frames=[A[40:45]] * 16), HOST_ONLY, "host-only"),
    *[(f"{k} sections", put(E, K=k), INVALID, "n_sections must be") for k in (0, -1, 17)],
    *[(f"hop {hop}", put(E, hop=hop), UNSUPPORTED, "power of two") for hop in (0, 32, 96, 480, 131072)],
    ("a frame short", put(E, count=COUNT - 1), INVALID, "n_frames must be"),
    ("the count of another hop", put(E, hop=128), INVALID, "n_frames must be"),
    ("frame stride below the count", put(E, fstride=COUNT - 1), INVALID, "frame_stride"),
    ("null frames", put(E, frames=None), INVALID, "null"),
    ("null in", put(E, x=0), INVALID, "null"),
    ("null out", put(E, out=0), INVALID, "null"),
    ("a null kept signal", put(EK, kept=[KEPT[0], 0]), INVALID, "kept 1"),
    *[(f"null frame array {i} of section {k}", put(E, frames=with_row(FRAMES, k, i, 0)), INVALID, f"frames {k}") for k in range(K) for i in (0, 4)],
    ("in 4 bytes off", put(E, x=X + 4), INVALID, "aligned"),
    ("a kept signal 4 bytes off", put(EK, kept=[KEPT[0] + 4, KEPT[1]]), INVALID, "aligned"),
    ("a frame array 4 bytes off is fine", put(E, frames=with_row(FRAMES, 1, 2, FRAMES[1][2] + 4)), HOST_ONLY, "host-only"),
    ("a frame array 2 bytes off", put(E, frames=with_row(FRAMES, 1, 2, FRAMES[1][2] + 2)), INVALID, "aligned"),
    ("in == out", put(E, out=X), INVALID, "in == out is not allowed"),
    ("out overlaps in", put(E, out=X + 16), INVALID, "overlaps in"),
    *[(f"out is frame array {i} of section {k}", put(E, out=FRAMES[k][i]), INVALID, f"overlaps frames of section {k} plane {i}")
      for k in range(K) for i in (0, 3)],
    ("out is a kept signal", put(EK, out=KEPT[1]), INVALID, "overlaps kept plane 1"),
    ("a kept signal is in", put(EK, kept=[X, KEPT[1]]), INVALID, "kept plane 0 overlaps in"),
    ("a kept signal is a frame array", put(EK, kept=[KEPT[0], FRAMES[2][1]]), INVALID, "kept plane 1 overlaps frames of section 2 plane 1"),
    ("the kept signals overlap", put(EK, kept=[KEPT[0], KEPT[0] + 16]), INVALID, "kept plane 0 overlaps kept plane 1"),
    # the header's order: sections, hop, count, stride, null, alignment, the overlaps
    ("the section count before the hop", put(E, K=0, hop=480), INVALID, "n_sections must be"),
    ("hop before the count", put(E, hop=480, count=1), UNSUPPORTED, "power of two"),
    ("the count before the stride", put(E, count=COUNT + 1, fstride=1), INVALID, "n_frames must be"),
    ("the stride before a null pointer", put(E, fstride=1, x=0), INVALID, "frame_stride"),
    ("null before alignment", put(E, x=X + 4, out=0), INVALID, "null"),
    ("alignment before overlap", put(E, x=X + 4, out=FRAMES[0][0]), INVALID, "aligned"),
    ("out before a kept signal", put(EK, out=X, kept=[X, KEPT[1]]), INVALID, "in == out"),
])
def test_execute_cascade_frames_refusals(what, a, status, text):
    got, message = raw_forward(a)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"


B = dict(EK, gout=GOUT, gin=GIN, grads=GRADS)
NO_GRADS = put(B, grads=None)
ALL_NULL = [[0] * 5 for _ in range(K)]


@pytest.mark.parametrize("what,a,status,text", [
    ("valid, with frame gradients", B, HOST_ONLY, "host-only"),
    ("valid, frame_grads null, nothing of the forward", put(NO_GRADS, x=0, out=0, kept=None), HOST_ONLY, "host-only"),
    ("valid, every frame gradient null, nothing of the forward", put(B, grads=ALL_NULL, x=0, out=0, kept=None), HOST_ONLY, "host-only"),
    ("grad_in is grad_out", put(B, gin=GOUT), HOST_ONLY, "host-only"),
    ("one section is the section's call", put(B, K=1), HOST_ONLY, "host-only"),
    *[(f"{k} sections", put(B, K=k), INVALID, "n_sections must be") for k in (0, 17)],
    ("hop 480", put(B, hop=480), UNSUPPORTED, "power of two"),
    ("a frame short", put(B, count=COUNT - 1), INVALID, "n_frames must be"),
    ("frame stride below the count", put(B, fstride=COUNT - 1), INVALID, "frame_stride"),
    ("null frames", put(B, frames=None), INVALID, "null"),
    *[(f"null {k}", put(B, **{k: 0}), INVALID, "null") for k in ("gout", "gin")],
    *[(f"frame gradients without {k}", put(B, **{k: 0}), INVALID, "null") for k in ("x", "out")],
    ("frame gradients without kept", put(B, kept=None), INVALID, "kept 0"),
    ("frame gradients without one kept signal", put(B, kept=[KEPT[0], 0]), INVALID, "kept 1"),
    ("a null frame array", put(B, frames=with_row(FRAMES, 2, 3, 0)), INVALID, "frames 2"),
    ("a frame gradient 2 bytes off", put(B, grads=with_row(GRADS, 1, 0, GRADS[1][0] + 2)), INVALID, "aligned"),
    *[(f"frame gradient {i} of section {k} alone missing", put(B, grads=with_row(GRADS, k, i, 0)), INVALID, "all given or all null")
      for k in (0, 2) for i in (0, 4)],
    ("one frame gradient alone given", put(B, grads=with_row(ALL_NULL, 1, 2, GRADS[1][2])), INVALID, "all given or all null"),
    ("the gradients of one section alone", put(B, grads=[GRADS[0], [0] * 5, [0] * 5]), INVALID, "every section alike"),
    ("grad_in is in", put(B, gin=X), INVALID, "grad_in plane 0 overlaps in"),
    ("grad_in is out", put(B, gin=OUT), INVALID, "grad_in plane 0 overlaps out"),
    ("grad_in is a kept signal", put(B, gin=KEPT[1]), INVALID, "grad_in plane 0 overlaps kept plane 1"),
    ("grad_in is a frame array", put(B, gin=FRAMES[1][3]), INVALID, "grad_in plane 0 overlaps frames of section 1 plane 3"),
    ("grad_in overlaps grad_out without being it", put(B, gin=GOUT + 16), INVALID, "overlaps grad_out"),
    ("a frame gradient is its frame array", put(B, grads=with_row(GRADS, 2, 1, FRAMES[2][1])), INVALID,
     "gradient of frames of section 2 plane 1 overlaps frames of section 2 plane 1"),
    ("a frame gradient is in", put(B, grads=with_row(GRADS, 0, 3, X)), INVALID, "gradient of frames of section 0 plane 3 overlaps in"),
    ("a frame gradient is a kept signal", put(B, grads=with_row(GRADS, 0, 3, KEPT[0])), INVALID, "overlaps kept plane 0"),
    ("a frame gradient is grad_out", put(B, grads=with_row(GRADS, 1, 0, GOUT)), INVALID, "overlaps grad_out"),
    ("two frame gradients of two sections are one", put(B, grads=with_row(GRADS, 2, 2, GRADS[0][0])), INVALID,
     "gradient of frames of section 0 plane 0 overlaps gradient of frames of section 2 plane 2"),
    ("a frame gradient is grad_in", put(B, grads=with_row(GRADS, 1, 4, GIN)), INVALID, "grad_in plane 0 overlaps gradient of frames of section 1 plane 4"),
    # the header's order
    ("the section count before the hop", put(B, K=17, hop=480), INVALID, "n_sections must be"),
    ("the stride before the mix", put(B, fstride=1, grads=with_row(GRADS, 0, 0, 0)), INVALID, "frame_stride"),
    ("null before the mix", put(B, gout=0, grads=with_row(GRADS, 0, 0, 0)), INVALID, "null"),
    ("the mix before an overlap", put(B, gin=X, grads=with_row(GRADS, 0, 0, 0)), INVALID, "all given or all null"),
])
def test_backward_cascade_frames_refusals(what, a, status, text):
    got, message = raw_backward(a)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"


def test_null_plan_is_refused():
    null, L = ctypes.c_void_p(), capi.lib()
    assert L.rf_var2_plan_execute_cascade_frames(null, null, None, 2, 64, 66, 66, null, None, null) == INVALID and L.rf_last_error_string()
    assert L.rf_var2_plan_backward_cascade_frames(null, null, None, 2, 64, 66, 66, None, null, null, null, None, null) == INVALID
