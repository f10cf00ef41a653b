"""CPU tests of the direct-form-I section on control-rate frames (rf_var2_plan_execute_biquad_frames / _backward_biquad_frames): the
yardsticks of tests/frames_loops.py pinned against central differences and the transpose identity, the frame count, the exported
symbols and queries, every refusal of a call in the header's order on a host-only plan, and the condition the cases' seeds are
chosen by -- the numpy replay of the kernels at or below half the GPU tests' bar.  No kernel is launched."""
import ctypes

import numpy as np
import pytest

import biquad_emulator as emu
import frames_cases as cases
import frames_loops as loops
import recfilter_amd as rfa
from recfilter_amd import capi

DIRECTIONS = [True, False]
NEW_SYMBOLS = ["rf_var2_frames_count", "rf_var2_expand_frames", "rf_var2_plan_execute_biquad_frames", "rf_var2_plan_execute_biquad_frames_timed",
               "rf_var2_plan_backward_biquad_frames", "rf_var2_plan_backward_biquad_frames_timed", "rf_var2_plan_biquad_frames_num_kernels",
               "rf_var2_plan_backward_biquad_frames_num_kernels", "rf_var2_plan_backward_biquad_frames_bytes"]


def name_of(causal):
    return "causal" if causal else "anticausal"


def host_plan(length, lines=1, causal=True, stride=None):
    return rfa.Var2Plan(length, lines=lines, causal=causal, device=capi.RF_DEVICE_HOST_ONLY, stride=stride)


# ---- the yardsticks ---------------------------------------------------------------------------------------------------------------
def test_expand_is_the_formula_and_hits_the_frames():
    rng = np.random.default_rng(1)
    f = rng.random((2, 5)) * 4 - 2
    c = loops.expand(f, 64, 200)
    assert c.shape == (2, 200)
    np.testing.assert_array_equal(c[:, ::64], f[:, :4])
    for n in (1, 63, 65, 199):
        j, k = divmod(n, 64)
        np.testing.assert_allclose(c[:, n], f[:, j] + k / 64 * (f[:, j + 1] - f[:, j]), rtol=0, atol=1e-15)
    c32 = loops.expand(f.astype(np.float32), 64, 200, np.float32)
    assert c32.dtype == np.float32 and np.max(np.abs(c32 - loops.expand(f.astype(np.float32), 64, 200))) < 3e-7
    np.testing.assert_array_equal(c32[:, ::64], f.astype(np.float32)[:, :4])


@pytest.mark.parametrize("hop,n", [(64, 200), (64, 4), (128, 4100), (4096, 8196)])
def test_contract_is_the_transpose_of_expand(hop, n):
    """<expand(f), g> == <f, contract(g)> in f64"""
    rng = np.random.default_rng(hop + n)
    count = loops.frames_count(n, hop)
    f, g = rng.random((3, count)) * 2 - 1, rng.random((3, n)) * 2 - 1
    left, right = float(np.sum(loops.expand(f, hop, n) * g)), float(np.sum(f * loops.contract(g, hop, count)))
    assert abs(left - right) <= 1e-12 * float(np.sum(np.abs(g))), (left, right)


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_frame_gradients_against_central_differences(causal):
    """the directional derivative of L = sum(g * y) along random directions in x and in each frame array, f64 (N = 200, H = 64)"""
    n, hop, h = 200, 64, 1e-6
    count = loops.frames_count(n, hop)
    rng = np.random.default_rng(200 + causal)
    x, g = (rng.random((2, n)) * 2 - 1 for _ in range(2))
    frames = [np.asarray(f, dtype=np.float64) for f in cases.frames_of("resonator", 2, count, hop, rng)]

    def loss(xx, ff):
        return float(np.sum(g * loops.forward(xx, ff, hop, causal)))
    y = loops.forward(x, frames, hop, causal)
    gx, *gf = loops.adjoint(x, frames, hop, y, g, causal)
    d = rng.random((2, n)) * 2 - 1
    assert abs((loss(x + h * d, frames) - loss(x - h * d, frames)) / (2 * h) - float(np.sum(gx * d))) < 1e-6
    for i, grad in enumerate(gf):
        assert grad.shape == (2, count) and np.all(grad != 0)
        d = rng.random((2, count)) * 2 - 1
        up, down = list(frames), list(frames)
        up[i], down[i] = frames[i] + h * d, frames[i] - h * d
        assert abs((loss(x, up) - loss(x, down)) / (2 * h) - float(np.sum(grad * d))) < 1e-6, f"frames {i}"


def test_frames_count():
    for hop in (64, 128, 4096, 65536):
        for length in (1, 4, hop - 4, hop, hop + 4, 5 * hop, 1 << 30):
            assert rfa.frames_count(length, hop) == -(-length // hop) + 1 == loops.frames_count(length, hop)
            assert capi.lib().rf_var2_frames_count(length, hop) == rfa.frames_count(length, hop)
    for hop in (0, -64, 1, 32, 63, 65, 96, 480, 131072):
        assert capi.lib().rf_var2_frames_count(4096, hop) == 0
        with pytest.raises(ValueError):
            rfa.frames_count(4096, hop)
    assert capi.lib().rf_var2_frames_count(0, 64) == 0
    assert [rfa.frames_count(n, 64) for n in (4, 60, 64, 68, 4100)] == [2, 2, 2, 3, 66]


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbols_and_front_end():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTED_SYMBOLS and getattr(L, name)
    assert capi.RF_ABI == 3 and b"abi 3" in L.rf_version()
    for name in ("biquad_scan_frames", "expand_frames", "frames_count"):
        assert name in rfa.__all__ and callable(getattr(rfa, name))
    for method in ("execute_biquad_frames", "execute_biquad_frames_timed", "backward_biquad_frames", "backward_biquad_frames_timed",
                   "apply_biquad_frames"):
        assert callable(getattr(rfa.Var2Plan, method))


@pytest.mark.parametrize("length,lines,stride", [(4, 1, 4), (4096, 1, 4096), (4100, 3, 4112), (1 << 30, 1, 1 << 30)])
def test_queries_of_host_only_plans(length, lines, stride):
    tiles = -(-length // 64)
    groups = -(-tiles // 64)
    with host_plan(length, lines, True, stride) as plan:
        assert plan.biquad_frames_num_kernels == 3
        assert plan.backward_biquad_frames_num_kernels(False) == 4 and plan.backward_biquad_frames_num_kernels(True) == 5
        lam = 4 * ((lines - 1) * stride + length)
        for hop in (64, 512, 1024, 4096, 65536):
            assert plan.backward_biquad_frames_bytes(hop) == lam + 80 * lines * -(-length // min(hop, 1024))
        assert plan.backward_biquad_frames_bytes(480) == 0
        assert plan.workspace_bytes == 4 * lines * (6 * (tiles + groups) + 2 * groups)      # unchanged
        assert plan.backward_biquad_bytes == lam and plan.biquad_num_kernels == 3
    null = ctypes.c_void_p()
    L = capi.lib()
    assert L.rf_var2_plan_biquad_frames_num_kernels(null) == 0 and L.rf_var2_plan_backward_biquad_frames_num_kernels(null, 1) == 0
    assert L.rf_var2_plan_backward_biquad_frames_bytes(null, 64) == 0


def test_host_only_plan_refuses_to_run_and_a_short_report_is_refused_first():
    with host_plan(4096) as plan:
        for call in (lambda: plan.execute_biquad_frames(None, None, 64), lambda: plan.execute_biquad_frames_timed(None, None, 64),
                     lambda: plan.backward_biquad_frames(None, None, 64, None, None), lambda: plan.backward_biquad_frames_timed(None, None, 64, None, None)):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == capi.RF_ERR_HIP and "host-only" in str(e.value)
        null, ms = ctypes.c_void_p(), (ctypes.c_float * 5)()
        L = capi.lib()
        assert L.rf_var2_plan_execute_biquad_frames_timed(plan._h, null, None, 64, 65, 65, null, null, ms, None, 2) == capi.RF_ERR_INVALID_ARG
        assert b"ms_out" in L.rf_last_error_string()
        assert L.rf_var2_plan_backward_biquad_frames_timed(plan._h, null, None, 64, 65, 65, null, null, null, None, null, ms, None, 3) == capi.RF_ERR_INVALID_ARG
        assert b"ms_out" in L.rf_last_error_string()
    assert L.rf_var2_plan_execute_biquad_frames(null, null, None, 64, 65, 65, null, null) == capi.RF_ERR_INVALID_ARG and L.rf_last_error_string()
    assert L.rf_var2_plan_backward_biquad_frames(null, null, None, 64, 65, 65, null, null, null, None, null) == capi.RF_ERR_INVALID_ARG


# ---- the refusals of a call, on addresses that are only numbers -----------------------------------------------------------------
LENGTH, LINES, STRIDE, HOP = 4100, 3, 4112, 64
COUNT = 66                                    # ceil(4100 / 64) + 1
FSTRIDE = COUNT + 2
SPAN = (2 * STRIDE + LENGTH) * 4
FSPAN = (2 * FSTRIDE + COUNT) * 4
A = [(i + 1) << 20 for i in range(14)]
INVALID, UNSUPPORTED = capi.RF_ERR_INVALID_ARG, capi.RF_ERR_UNSUPPORTED


def section(addresses):
    return (capi.Var2Section * 1)(capi.Var2Section(*addresses)) if addresses is not None else None


def put(base, **at):
    out = dict(base)
    out.update(at)
    return out


def raw_forward(a):
    with host_plan(LENGTH, LINES, True, STRIDE) as plan:
        status = capi.lib().rf_var2_plan_execute_biquad_frames(plan._h, ctypes.c_void_p(a["x"]), section(a["frames"]), a["hop"], a["count"],
                                                               a["fstride"], ctypes.c_void_p(a["out"]), None)
        return status, capi.lib().rf_last_error_string().decode()


def raw_backward(a):
    with host_plan(LENGTH, LINES, True, STRIDE) as plan:
        status = capi.lib().rf_var2_plan_backward_biquad_frames(
            plan._h, ctypes.c_void_p(a["x"]), section(a["frames"]), a["hop"], a["count"], a["fstride"], ctypes.c_void_p(a["out"]),
            ctypes.c_void_p(a["gout"]), ctypes.c_void_p(a["gin"]), section(a["grads"]), None)
        return status, capi.lib().rf_last_error_string().decode()


def frames_with(i, value):
    f = A[1:6]
    f[i] = value
    return f


E = dict(x=A[0], frames=A[1:6], hop=HOP, count=COUNT, fstride=FSTRIDE, out=A[6])


@pytest.mark.parametrize("what,a,status,text", [
    ("valid: only the host-only refusal is left", E, capi.RF_ERR_HIP, "host-only"),
    ("a dense frame stride", put(E, fstride=COUNT), capi.RF_ERR_HIP, "host-only"),
    *[(f"hop {hop}", put(E, hop=hop), UNSUPPORTED, "power of two") for hop in (0, 32, 96, 480, 131072)],
    ("a frame short", put(E, count=COUNT - 1), INVALID, "n_frames must be"),
    ("a frame long", put(E, count=COUNT + 1, fstride=COUNT + 1), INVALID, "n_frames must be"),
    ("the count of another hop", put(E, hop=128), INVALID, "n_frames must be"),
    ("frame stride below the count", put(E, fstride=COUNT - 1), INVALID, "frame_stride"),
    ("null frames", put(E, frames=None), INVALID, "null"),
    ("null in", put(E, x=0), INVALID, "null"),
    ("null out", put(E, out=0), INVALID, "null"),
    *[(f"null frame array {i}", put(E, frames=frames_with(i, 0)), INVALID, "null") for i in range(5)],
    ("in 4 bytes off", put(E, x=A[0] + 4), INVALID, "aligned"),
    ("a frame array 4 bytes off is fine", put(E, frames=frames_with(2, A[3] + 4)), capi.RF_ERR_HIP, "host-only"),
    ("a frame array 2 bytes off", put(E, frames=frames_with(2, A[3] + 2)), INVALID, "aligned"),
    ("in == out", put(E, out=A[0]), INVALID, "in == out is not allowed"),
    ("out overlaps in", put(E, out=A[0] + 16), INVALID, "overlaps in"),
    *[(f"out is frame array {i}", put(E, out=A[1 + i]), INVALID, f"overlaps frames plane {i}") for i in range(5)],
    ("out ends inside a2's frames", put(E, out=A[5] - SPAN + 16), INVALID, "overlaps frames plane 4"),
    ("out begins at b0's last frame", put(E, frames=frames_with(0, A[9] + 12), out=A[9] + FSPAN + 8), INVALID, "overlaps frames plane 0"),
    ("out begins behind b0's last frame", put(E, frames=frames_with(0, A[9] + 8), out=A[9] + FSPAN + 8), capi.RF_ERR_HIP, "host-only"),
    # the header's order: hop, count, stride, null, the overlaps
    ("hop before the count", put(E, hop=480, count=1), UNSUPPORTED, "power of two"),
    ("the count before the stride", put(E, count=COUNT + 1, fstride=1), INVALID, "n_frames must be"),
    ("the stride before a null pointer", put(E, fstride=1, x=0), INVALID, "frame_stride"),
    ("null before alignment", put(E, x=A[0] + 4, out=0), INVALID, "null"),
    ("alignment before overlap", put(E, x=A[0] + 4, out=A[1]), INVALID, "aligned"),
    ("in before a frame array", put(E, x=A[1], out=A[1]), INVALID, "in == out"),
])
def test_execute_biquad_frames_refusals(what, a, status, text):
    got, message = raw_forward(a)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"


B = dict(E, gout=A[7], gin=A[8], grads=A[9:14])
NO_GRADS = put(B, grads=None)


def grads_with(i, value, base=None):
    g = list(base) if base is not None else A[9:14]
    g[i] = value
    return g


@pytest.mark.parametrize("what,a,status,text", [
    ("valid, with frame gradients", B, capi.RF_ERR_HIP, "host-only"),
    ("valid, frame_grads null, no out", put(NO_GRADS, out=0), capi.RF_ERR_HIP, "host-only"),
    ("valid, five null frame gradients, no out", put(B, grads=[0] * 5, out=0), capi.RF_ERR_HIP, "host-only"),
    ("grad_in is grad_out", put(B, gin=A[7]), capi.RF_ERR_HIP, "host-only"),
    ("hop 480", put(B, hop=480), UNSUPPORTED, "power of two"),
    ("a frame short", put(B, count=COUNT - 1), INVALID, "n_frames must be"),
    ("frame stride below the count", put(B, fstride=COUNT - 1), INVALID, "frame_stride"),
    *[(f"null {k}", put(B, **{k: 0}), INVALID, "null") for k in ("x", "gout", "gin")],
    ("null frames", put(B, frames=None), INVALID, "null"),
    ("frame gradients without out", put(B, out=0), INVALID, "null"),
    *[(f"frame gradient {i} alone missing", put(B, grads=grads_with(i, 0)), INVALID, "all given or all null") for i in range(5)],
    *[(f"frame gradient {i} alone given", put(B, grads=grads_with(i, A[9 + i], [0] * 5)), INVALID, "all given or all null") for i in range(5)],
    ("grad_in is in", put(B, gin=A[0]), INVALID, "grad_in plane 0 overlaps in"),
    ("grad_in is out", put(B, gin=A[6]), INVALID, "grad_in plane 0 overlaps out"),
    ("grad_in is a1's frames", put(B, gin=A[4]), INVALID, "grad_in plane 0 overlaps frames plane 3"),
    ("grad_in overlaps grad_out without being it", put(B, gin=A[7] + 16), INVALID, "overlaps grad_out"),
    ("grad of b1 is b1", put(B, grads=grads_with(1, A[2])), INVALID, "gradient of frames plane 1 overlaps frames plane 1"),
    ("grad of a1 is in", put(B, grads=grads_with(3, A[0])), INVALID, "gradient of frames plane 3 overlaps in"),
    ("grad of b0 is grad_out", put(B, grads=grads_with(0, A[7])), INVALID, "overlaps grad_out"),
    ("grad of b2 is grad of b0", put(B, grads=grads_with(2, A[9])), INVALID, "overlaps gradient of frames"),
    ("grad of a2 is grad_in", put(B, grads=grads_with(4, A[8])), INVALID, "overlaps gradient of frames"),
    # the header's order: a null pointer before the mix before the overlaps
    ("null before the mix", put(B, x=0, grads=grads_with(0, 0)), INVALID, "null"),
    ("the mix before an overlap", put(B, gin=A[0], grads=grads_with(0, 0)), INVALID, "all given or all null"),
    ("the stride before the mix", put(B, fstride=1, grads=grads_with(0, 0)), INVALID, "frame_stride"),
])
def test_backward_biquad_frames_refusals(what, a, status, text):
    got, message = raw_backward(a)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"


@pytest.mark.parametrize("what,kw,status,text", [
    ("hop", dict(hop=480), UNSUPPORTED, "power of two"),
    ("count", dict(count=COUNT + 1), INVALID, "n_frames must be"),
    ("frame stride", dict(fstride=COUNT - 1), INVALID, "frame_stride"),
    ("length", dict(length=4098), INVALID, "multiple of 4"),
    ("stride", dict(stride=4096), INVALID, "stride"),
    ("null frames", dict(frames=0), INVALID, "null"),
    ("null out", dict(out=0), INVALID, "null"),
    ("out off", dict(out=A[1] + 4), INVALID, "aligned"),
    ("out is the frames", dict(out=A[0]), INVALID, "overlaps"),
])
def test_expand_frames_refusals(what, kw, status, text):
    """no device is touched before the last check: these run without one"""
    a = dict(frames=A[0], hop=HOP, count=COUNT, fstride=FSTRIDE, length=LENGTH, lines=LINES, stride=STRIDE, out=A[1])
    a.update(kw)
    got = capi.lib().rf_var2_expand_frames(ctypes.c_void_p(a["frames"]), a["hop"], a["count"], a["fstride"], a["length"], a["lines"], a["stride"],
                                           ctypes.c_void_p(a["out"]), None)
    message = capi.lib().rf_last_error_string().decode()
    assert got == status and text in message, f"{what}: status {got} ({message})"


# ---- the seeds ----------------------------------------------------------------------------------------------------------------------
def replay(hop, n, lines, kind, causal):
    """the kernels' arithmetic in numpy: the f32 expansion, tests/biquad_emulator.py's launches on it, the five per-sample
    gradients contracted in f64 and rounded once to f32"""
    x, frames, g = cases.case(hop, n, lines, kind, causal)
    count = loops.frames_count(n, hop)
    signals = loops.expand_all(frames, hop, n, np.float32)
    got = {name: np.empty((lines, n if name in ("out", "grad_x") else count), np.float32) for name in cases.NAMES}
    for l in range(lines):
        one = [s[l] for s in signals]
        y = emu.tiled_forward(x[l], *one, causal)
        gx, *per_sample = emu.tiled_adjoint(x[l], *one, y, g[l], causal)
        got["out"][l], got["grad_x"][l] = y, gx
        for name, p in zip(cases.NAMES[2:], per_sample):
            got[name][l] = loops.contract(p, hop, count, np.float64).astype(np.float32)
    return got


@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("hop,n,lines", cases.SHAPES)
def test_replay_at_or_below_half_the_bar_on_every_gpu_case(hop, n, lines, kind, causal):
    """what the seeds of tests/frames_cases.py are chosen by: forward, grad_x and the five frame gradients of the numpy replay"""
    want = cases.expected(hop, n, lines, kind, causal)
    got = replay(hop, n, lines, kind, causal)
    for name in cases.NAMES:
        cases.assert_under_half_the_bar(got[name], want[name], f"replay hop {hop} {n} x {lines} {kind} {name_of(causal)} {name}")
