"""CPU tests of the time-varying second-order all-pole scans (rf_var2_plan_*): host-only plans -- creation, launch counts, the
workspace formula, every refusal with its status and text -- the loops of tests/var2_loops.py pinned by central differences, and
the tiled algebra of kernels_var2_signal.hip replayed in numpy f32 (tests/var2_emulator.py) under the GPU tests' bar on every
case the GPU tests use -- at or below half of it on the long-memory cases, whose seeds are chosen by that, and exact on the integer
rotations of tests/var2_exact.py, whose closed form is pinned against the loops here.  No kernel is launched."""
import ctypes

import numpy as np
import pytest

import var2_cases as cases
import var2_emulator as emu
import var2_exact as exact
import var2_loops as loops
import recfilter_amd as rfa
from recfilter_amd import capi


def host_plan(length, lines=1, causal=True, stride=None):
    return rfa.Var2Plan(length, lines=lines, causal=causal, device=capi.RF_DEVICE_HOST_ONLY, stride=stride)


def raw_create(edit):
    """rf_var2_plan_create_signal on a valid host-only description of 4096 samples after edit(desc); returns (status, message)"""
    d = capi.Var2SignalDesc()
    d.abi, d.length, d.n_lines, d.stride, d.causal = capi.RF_ABI, 4096, 1, 4096, 1
    d.device, d.flags = capi.RF_DEVICE_HOST_ONLY, 0
    edit(d)
    h = ctypes.c_void_p()
    status = capi.lib().rf_var2_plan_create_signal(ctypes.byref(d), ctypes.byref(h))
    message = capi.lib().rf_last_error_string().decode()
    if status == capi.RF_OK:
        capi.lib().rf_var2_plan_destroy(h)
    else:
        assert not h.value, "a refused description must not leave a plan behind"
    return status, message


def set_fields(**fields):
    def edit(d):
        for name, value in fields.items():
            setattr(d, name, value)
    return edit


# ---- host-only plans ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fields", [dict(length=4, stride=4), dict(length=10_000_000, stride=10_000_000), dict(length=1 << 30, stride=1 << 30),
                                    dict(n_lines=65535), dict(stride=4100, n_lines=3), dict(causal=0)])
def test_valid_description_is_accepted(fields):
    status, message = raw_create(set_fields(**fields))
    assert status == capi.RF_OK, message


@pytest.mark.parametrize("what,fields,status,text", [
    ("abi", dict(abi=capi.RF_ABI - 1), capi.RF_ERR_INVALID_ARG, "abi"),
    ("flags", dict(flags=1), capi.RF_ERR_INVALID_ARG, "flags"),
    ("length 0", dict(length=0), capi.RF_ERR_INVALID_ARG, "length"),
    ("length -4", dict(length=-4), capi.RF_ERR_INVALID_ARG, "length"),
    ("n_lines 0", dict(n_lines=0), capi.RF_ERR_INVALID_ARG, "n_lines"),
    ("n_lines 65536", dict(n_lines=65536), capi.RF_ERR_INVALID_ARG, "n_lines"),
    ("stride below the length", dict(stride=4092), capi.RF_ERR_INVALID_ARG, "stride"),
    ("stride 4098", dict(stride=4098), capi.RF_ERR_INVALID_ARG, "stride"),
    ("length 6", dict(length=6, stride=8), capi.RF_ERR_UNSUPPORTED, "multiple of 4"),
    ("length 4099", dict(length=4099, stride=4100), capi.RF_ERR_UNSUPPORTED, "multiple of 4"),
    ("length 2^30 + 4", dict(length=(1 << 30) + 4, stride=(1 << 30) + 4), capi.RF_ERR_UNSUPPORTED, "2^30"),
    # the stated order: abi before flags before the extents; bad extents before the unsupported lengths
    ("abi first", dict(abi=0, flags=1, length=6), capi.RF_ERR_INVALID_ARG, "abi"),
    ("flags before length", dict(flags=2, length=0), capi.RF_ERR_INVALID_ARG, "flags"),
    ("n_lines before an unsupported length", dict(length=6, stride=8, n_lines=0), capi.RF_ERR_INVALID_ARG, "n_lines"),
])
def test_create_refusals(what, fields, status, text):
    got, message = raw_create(set_fields(**fields))
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: the message does not name the field: {message!r}"


def test_null_arguments_are_refused():
    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.rf_var2_plan_create_signal(None, ctypes.byref(h)) == capi.RF_ERR_INVALID_ARG and L.rf_last_error_string() and not h.value
    d = capi.Var2SignalDesc()
    assert L.rf_var2_plan_create_signal(ctypes.byref(d), None) == capi.RF_ERR_INVALID_ARG and L.rf_last_error_string()
    null = ctypes.c_void_p()
    assert L.rf_var2_plan_execute(null, null, null, null, null, null) == capi.RF_ERR_INVALID_ARG and L.rf_last_error_string()
    assert L.rf_var2_plan_backward(null, null, null, null, null, null, null, null, null) == capi.RF_ERR_INVALID_ARG and L.rf_last_error_string()
    ms = (ctypes.c_float * 4)()
    assert L.rf_var2_plan_execute_timed(null, null, null, null, null, null, ms, None, 4) == capi.RF_ERR_INVALID_ARG
    assert L.rf_var2_plan_backward_timed(null, null, null, null, null, null, null, null, null, ms, None, 4) == capi.RF_ERR_INVALID_ARG
    assert L.rf_var2_plan_num_kernels(null) == 0 and L.rf_var2_plan_workspace_bytes(null) == 0
    assert L.rf_var2_plan_backward_num_kernels(null, 1) == 0
    assert L.rf_var2_plan_destroy(null) == capi.RF_OK


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("length,lines", [(4, 1), (4096, 1), (4100, 3), (1 << 30, 1), (1 << 30, 65535)])
def test_queries_of_host_only_plans(length, lines, causal):
    tiles = -(-length // 64)
    groups = -(-tiles // 64)
    with host_plan(length, lines, causal) as plan:
        assert plan.num_kernels == 3
        assert plan.backward_num_kernels(False) == 3
        assert plan.backward_num_kernels(True) == 4
        assert plan.workspace_bytes == 4 * lines * (6 * (tiles + groups) + 2 * groups)


def test_host_only_plan_refuses_to_run_and_a_short_report_is_refused_first():
    with host_plan(4096) as plan:
        for call in (lambda: plan.execute(None, None, None), lambda: plan.execute_timed(None, None, None),
                     lambda: plan.backward(None, None, None, None), lambda: plan.backward_timed(None, None, None, None)):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == capi.RF_ERR_HIP and "host-only" in str(e.value)
        null, ms = ctypes.c_void_p(), (ctypes.c_float * 2)()
        assert capi.lib().rf_var2_plan_execute_timed(plan._h, null, null, null, null, null, ms, None, 2) == capi.RF_ERR_INVALID_ARG
        assert b"ms_out" in capi.lib().rf_last_error_string()


# a call's arguments are checked before the host-only refusal and never dereferenced: addresses that are only numbers
SPAN = (2 * 4112 + 4100) * 4      # 3 lines of 4100 samples, 4112 apart
A = [1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20, 7 << 20]


def raw_call(name, *addresses):
    """(status, message) of rf_var2_plan_execute / _backward on a host-only plan of 3 x 4100 samples with these addresses"""
    with host_plan(4100, 3, True, 4112) as plan:
        status = getattr(capi.lib(), name)(plan._h, *(ctypes.c_void_p(a) for a in addresses), None)
        return status, capi.lib().rf_last_error_string().decode()


@pytest.mark.parametrize("what,addresses,status,text", [
    ("valid: only the host-only refusal is left", A[:4], capi.RF_ERR_HIP, "host-only"),
    ("in place", [A[0], A[1], A[2], A[0]], capi.RF_ERR_HIP, "host-only"),
    ("null in", [0] + A[1:4], capi.RF_ERR_INVALID_ARG, "null"),
    ("null a1", [A[0], 0, A[2], A[3]], capi.RF_ERR_INVALID_ARG, "null"),
    ("null a2", [A[0], A[1], 0, A[3]], capi.RF_ERR_INVALID_ARG, "null"),
    ("null out", A[:3] + [0], capi.RF_ERR_INVALID_ARG, "null"),
    ("in 4 bytes off", [A[0] + 4] + A[1:4], capi.RF_ERR_INVALID_ARG, "aligned"),
    ("out 8 bytes off", A[:3] + [A[3] + 8], capi.RF_ERR_INVALID_ARG, "aligned"),
    ("out is a1", [A[0], A[1], A[2], A[1]], capi.RF_ERR_INVALID_ARG, "coefficient"),
    ("out reaches into a2", [A[0], A[1], A[2], A[2] - SPAN + 16], capi.RF_ERR_INVALID_ARG, "coefficient"),
    ("out overlaps in without being it", [A[0], A[1], A[2], A[0] + 16], capi.RF_ERR_INVALID_ARG, "overlaps in"),
])
def test_execute_refusals(what, addresses, status, text):
    got, message = raw_call("rf_var2_plan_execute", *addresses)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"


# (a1, a2, out, grad_out, grad_in, grad_a1, grad_a2)
@pytest.mark.parametrize("what,addresses,status,text", [
    ("valid, no coefficient gradients, no out", [A[0], A[1], 0, A[3], A[4], 0, 0], capi.RF_ERR_HIP, "host-only"),
    ("valid, with coefficient gradients", A, capi.RF_ERR_HIP, "host-only"),
    ("in place", [A[0], A[1], A[2], A[3], A[3], A[5], A[6]], capi.RF_ERR_HIP, "host-only"),
    ("grad_a1 without grad_a2", A[:6] + [0], capi.RF_ERR_INVALID_ARG, "grad_a1 and grad_a2"),
    ("grad_a2 without grad_a1", A[:5] + [0, A[6]], capi.RF_ERR_INVALID_ARG, "grad_a1 and grad_a2"),
    ("null a1", [0] + A[1:], capi.RF_ERR_INVALID_ARG, "null"),
    ("null a2", [A[0], 0] + A[2:], capi.RF_ERR_INVALID_ARG, "null"),
    ("null grad_out", A[:3] + [0] + A[4:], capi.RF_ERR_INVALID_ARG, "null"),
    ("null grad_in", A[:4] + [0] + A[5:], capi.RF_ERR_INVALID_ARG, "null"),
    ("coefficient gradients without out", A[:2] + [0] + A[3:], capi.RF_ERR_INVALID_ARG, "null"),
    ("grad_a2 4 bytes off", A[:6] + [A[6] + 4], capi.RF_ERR_INVALID_ARG, "aligned"),
    ("grad_in is a1", A[:4] + [A[0]] + A[5:], capi.RF_ERR_INVALID_ARG, "grad_in plane 0 overlaps coefficient"),
    ("grad_in overlaps grad_out without being it", A[:4] + [A[3] + 16] + A[5:], capi.RF_ERR_INVALID_ARG, "overlaps grad_out"),
    ("grad_a1 is out", A[:5] + [A[2], A[6]], capi.RF_ERR_INVALID_ARG, "overlaps out"),
    ("grad_a2 is grad_out", A[:6] + [A[3]], capi.RF_ERR_INVALID_ARG, "overlaps grad_out"),
    ("grad_a2 is grad_a1", A[:6] + [A[5]], capi.RF_ERR_INVALID_ARG, "overlaps gradient of coefficient"),
    ("grad_a1 is grad_in", A[:5] + [A[4], A[6]], capi.RF_ERR_INVALID_ARG, "overlaps gradient of coefficient"),
])
def test_backward_refusals(what, addresses, status, text):
    got, message = raw_call("rf_var2_plan_backward", *addresses)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"


def test_abi_revision_is_unchanged():
    assert capi.RF_ABI == 3
    assert b"abi 3" in capi.lib().rf_version()
    for name in ("rf_var2_plan_create_signal", "rf_var2_plan_execute", "rf_var2_plan_backward", "rf_var2_plan_backward_num_kernels"):
        assert name in capi.EXPORTED_SYMBOLS


# ---- the loops ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_adjoint_loops_against_central_differences(causal):
    """the directional derivative of L = sum(g * y) along random directions in x, a1 and a2, f64; the masked slots get 0"""
    n, h = 68, 1e-6
    rng = np.random.default_rng(68 + causal)
    x, g, dx, d1, d2 = (rng.random((2, n)) * 2 - 1 for _ in range(5))
    a1, a2 = (np.asarray(a, dtype=np.float64) for a in cases.coefficients("resonator", (2, n), rng))

    def loss(xx, aa1, aa2):
        return float(np.sum(g * loops.forward(xx, aa1, aa2, causal, np.float64)))
    y = loops.forward(x, a1, a2, causal, np.float64)
    gx, g1, g2 = loops.adjoint(a1, a2, y, g, causal, np.float64)
    assert abs((loss(x + h * dx, a1, a2) - loss(x - h * dx, a1, a2)) / (2 * h) - float(np.sum(gx * dx))) < 1e-6
    assert abs((loss(x, a1 + h * d1, a2) - loss(x, a1 - h * d1, a2)) / (2 * h) - float(np.sum(g1 * d1))) < 1e-6
    assert abs((loss(x, a1, a2 + h * d2) - loss(x, a1, a2 - h * d2)) / (2 * h) - float(np.sum(g2 * d2))) < 1e-6
    first, second = (np.s_[:, :1], np.s_[:, :2]) if causal else (np.s_[:, -1:], np.s_[:, -2:])
    assert np.all(g1[first] == 0) and np.all(g2[second] == 0)
    assert np.any(g1 != 0) and np.any(g2 != 0)


@pytest.mark.parametrize("causal", [True, False])
def test_a_nan_in_a_masked_slot_reaches_nothing(causal):
    x, a1, a2, g = cases.case(68, 1, "resonator", causal)
    assert np.isnan(a1).sum() == 1 and np.isnan(a2).sum() == 2
    y = loops.forward(x, a1, a2, causal)
    assert not np.isnan(y).any() and not any(np.isnan(r).any() for r in loops.adjoint(a1, a2, y, g, causal))
    assert not np.isnan(emu.tiled_forward(x[0], a1[0], a2[0], causal)).any()


@pytest.mark.parametrize("causal", [True, False])
def test_segmented_loops_are_the_loops(causal):
    """on a sprinkled line of 8196 samples, f64: the segments give the serial loop's values to rounding"""
    x, a1, a2, g = cases.case(8196, 1, "sprinkled", causal)
    a1m, a2m = (a1[0], a2[0]) if causal else (a1[0][::-1], a2[0][::-1])
    assert len(loops.segment_starts(*loops.masked(a1m, a2m, np.float64))) > 10
    y = loops.forward(x, a1, a2, causal)
    np.testing.assert_allclose(loops.segmented_forward(x[0], a1[0], a2[0], causal), y[0], rtol=0, atol=1e-12)
    for got, want in zip(loops.segmented_adjoint(a1[0], a2[0], y[0], g[0], causal), loops.adjoint(a1, a2, y, g, causal)):
        np.testing.assert_allclose(got, want[0], rtol=0, atol=1e-10)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("n", [4098, 4097, 7])
def test_padding_rule_of_allpole_scan(n, causal):
    """zeros behind the end of a causal scan, before the start of an anticausal one: the real samples are the unpadded scan's, and
    so are their gradients (the loops take any length)"""
    rng = np.random.default_rng(n)
    x, g = (rng.random(n) * 2 - 1 for _ in range(2))
    a1, a2 = (np.asarray(a, dtype=np.float64) for a in cases.coefficients("resonator", (n,), rng))
    pad = -n % 4
    where = (0, pad) if causal else (pad, 0)
    keep = np.s_[:n] if causal else np.s_[pad:]
    px, p1, p2, pg = (np.pad(a, where) for a in (x, a1, a2, g))
    y = loops.forward(x, a1, a2, causal)
    py = loops.forward(px, p1, p2, causal)
    np.testing.assert_array_equal(py[keep], y)
    for got, want in zip(loops.adjoint(p1, p2, py, pg, causal), loops.adjoint(a1, a2, y, g, causal)):
        np.testing.assert_array_equal(got[keep], want)


# ---- the tiled algebra ------------------------------------------------------------------------------------------------------------
def test_compose_is_associative_to_rounding():
    rng = np.random.default_rng(5)
    n = 4096
    raw = [tuple(rng.random(n) * 2 - 1 for _ in range(6)) for _ in range(3)]

    def f64_compose(A, B):
        ae0, ae1, a00, a01, a10, a11 = A
        be0, be1, b00, b01, b10, b11 = B
        return (be0 + b00 * ae0 + b01 * ae1, be1 + b10 * ae0 + b11 * ae1, b00 * a00 + b01 * a10, b00 * a01 + b01 * a11,
                b10 * a00 + b11 * a10, b10 * a01 + b11 * a11)
    a, b, c = [tuple(v.astype(np.float32) for v in t) for t in raw]
    A, B, C = [tuple(v.astype(np.float64) for v in t) for t in (a, b, c)]
    left, right = f64_compose(f64_compose(A, B), C), f64_compose(A, f64_compose(B, C))
    for l, r in zip(left, right):
        np.testing.assert_allclose(l, r, rtol=0, atol=1e-14)
    for got in (emu.compose(emu.compose(a, b), c), emu.compose(a, emu.compose(b, c))):
        for v, want in zip(got, left):
            assert v.dtype == np.float32
            # a component is a sum of at most 7 products of three values in [-1, 1]: magnitudes below 7, a handful of roundings
            np.testing.assert_allclose(v, want, rtol=0, atol=16 * 2.0 ** -24 * 7)
    e = emu.identity((n,))
    for got in (emu.compose(e, a), emu.compose(a, e)):
        for v, want in zip(got, a):
            np.testing.assert_array_equal(v, want)


@pytest.mark.parametrize("causal", [True, False])
def test_tile_tails_and_carries_are_the_serial_states(causal):
    """E and P of the algebra mean what the design says: the state that enters every tile, formed from maps and carries, is the
    serial loop's (y[t0-1], y[t0-2]) to rounding"""
    n = 3 * 4096 + 68
    x, a1, a2, _ = cases.case(12356, 1, "resonator", causal)
    assert x.shape[1] == n
    parts = {}
    emu.tiled_scan(x[0], a1[0], a2[0], causal, False, parts)
    y = loops.forward(x, a1, a2, causal)[0]
    y = y if causal else y[::-1]
    # the samples the last group lacks are zeros: behind the line, or (the padded line reversed) before its real samples
    y = np.concatenate([y, np.zeros(4 * 4096 - n)] if causal else [np.zeros(4 * 4096 - n), y])
    starts = np.arange(0, 4 * 4096, 64)
    prev1 = np.where(starts >= 1, y[np.maximum(starts - 1, 0)], 0)
    prev2 = np.where(starts >= 2, y[np.maximum(starts - 2, 0)], 0)
    scale = float(np.max(np.abs(y)))
    np.testing.assert_allclose(parts["enter"][0].reshape(-1), prev1, rtol=0, atol=2e-5 * scale)
    np.testing.assert_allclose(parts["enter"][1].reshape(-1), prev2, rtol=0, atol=2e-5 * scale)


GPU_CASES = ([(n, 1, kind) for n in cases.LENGTHS for kind in cases.KINDS] + [(n, lines, "resonator") for lines, n, _ in cases.LINE_CASES]
             + [(cases.LONG, 1, "sprinkled")] + cases.LONG_MEMORY_CASES)


def replay(n, lines, kind, causal):
    x, a1, a2, g = cases.case(n, lines, kind, causal)
    got = {name: np.empty((lines, n), np.float32) for name in ("out", "grad_x", "grad_a1", "grad_a2")}
    for l in range(lines):
        y = emu.tiled_forward(x[l], a1[l], a2[l], causal)
        got["out"][l] = y
        got["grad_x"][l], got["grad_a1"][l], got["grad_a2"][l] = emu.tiled_adjoint(a1[l], a2[l], y, g[l], causal)
    return got


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("n,lines,kind", GPU_CASES)
def test_emulator_under_the_bar_on_every_gpu_case(n, lines, kind, causal):
    """what makes the GPU tests ones the algebra itself passes: forward and all three gradients of the numpy f32 replay"""
    want = cases.expected(n, lines, kind, causal)
    got = replay(n, lines, kind, causal)
    for name in want:
        cases.assert_under_bar(got[name], want[name], f"emulator {n} x {lines} {kind} {'causal' if causal else 'anticausal'} {name}")


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("n,lines,kind", cases.LONG_MEMORY_CASES)
def test_emulator_under_half_the_bar_on_every_long_memory_case(n, lines, kind, causal):
    """the condition the seeds of cases.LONG_MEMORY_SEEDS were chosen by: a kernel result above the bar on one of these cases is
    then a finding about the kernel, not about the draw"""
    assert set(cases.LONG_MEMORY_SEEDS) == {(n, kind, c) for n, _, kind in cases.LONG_MEMORY_CASES for c in (True, False)}
    want = cases.expected(n, lines, kind, causal)
    got = replay(n, lines, kind, causal)
    for name in want:
        cases.assert_under_half_the_bar(got[name], want[name], f"emulator {n} x {lines} {kind} {'causal' if causal else 'anticausal'} {name}")


def test_long_memory_family_keeps_its_memory():
    """r inside [0.998, 0.9995], and the long case's cuts 20,000 .. 40,000 samples apart, none near a sweep boundary (the case
    itself asserts the latter): about 140 lines for the segmented loops"""
    for n, _, kind in cases.LONG_MEMORY_CASES:
        _, a1, a2, _ = cases.case(n, 1, kind, True)
        r = np.sqrt(a2[0][2:].astype(np.float64))
        live = r > 0
        assert r[live].min() >= 0.998 - 1e-6 and r[live].max() <= 0.9995 + 1e-6
        if kind == "long memory, cut":
            starts = loops.segment_starts(*loops.masked(a1[0], a2[0], np.float64))
            gaps = np.diff(starts)
            gaps = gaps[gaps > 1]      # (a cut decouples at two neighbouring samples: a segment of one sample before each long one)
            assert 100 <= len(gaps) <= 220 and gaps.min() >= 20000 - 1 and gaps.max() <= 40000
        else:
            assert live.all()


# ---- the exact cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", list(exact.FAMILIES))
@pytest.mark.parametrize("n", [4, 68, 4100, 12292])
def test_integer_closed_forms_are_the_serial_loops(n, family, causal):
    """tests/var2_exact.py against the f64 loops, ends included: the all-pole scan, the section with integer taps, and (period 6
    into period 3) the cascade of two"""
    import biquad_loops
    import cascade_loops
    x, a1, a2, g = exact.case(n, family, causal)
    want = exact.expected(n, family, causal)
    y = loops.forward(x, a1, a2, causal)
    np.testing.assert_array_equal(y, want["out"])
    for got, name in zip(loops.adjoint(a1, a2, y, g, causal), ("grad_x", "grad_a1", "grad_a2")):
        np.testing.assert_array_equal(got, want[name], name)
    if n > 4:
        assert all(np.any(want[name] != 0) for name in want)
    signals = exact.biquad_case(n, family, causal)
    want = exact.biquad_expected(n, family, causal)
    y = biquad_loops.forward(*signals[:6], causal)
    for got, name in zip((y, *biquad_loops.adjoint(*signals[:6], y, signals[6], causal)), want):
        np.testing.assert_array_equal(got, want[name], name)
    if family == "period 6":
        x, sections, g = exact.cascade_case(n, causal)
        want, left_out = exact.cascade_expected(n, causal)
        assert not left_out
        ys = cascade_loops.forward(x, sections, causal)
        got = dict(zip(cascade_names(2), cascade_flat(ys[-1], cascade_loops.adjoint(x, sections, ys, g, causal))))
        assert set(got) == set(want)
        for name in want:
            np.testing.assert_array_equal(got[name], want[name], name)


def cascade_names(K):
    return ("out", "grad_x") + tuple(f"grad_{c}_{k}" for k in range(K) for c in exact.COEFFICIENTS)


def cascade_flat(result, grads):
    return [result, grads[0]] + [c for s in grads[1] for c in s]


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", list(exact.FAMILIES))
@pytest.mark.parametrize("n", exact.LENGTHS)
def test_emulator_is_exact_on_every_exact_gpu_case(n, family, causal):
    """the numpy f32 replay gives the integers: forward and all three gradients, no tolerance"""
    x, a1, a2, g = exact.case(n, family, causal)
    want = exact.expected(n, family, causal)
    y = emu.tiled_forward(x[0], a1[0], a2[0], causal)
    for got, name in zip((y, *emu.tiled_adjoint(a1[0], a2[0], y, g[0], causal)), ("out", "grad_x", "grad_a1", "grad_a2")):
        np.testing.assert_array_equal(got, want[name][0], name)


def test_exact_families_are_the_integer_rotations():
    """the companion matrices: period 6 and 3 (no power of two: M^64 and M^4096 are not the identity and not symmetric), and the
    running sum's singular one"""
    for family, period in (("period 6", 6), ("period 3", 3), ("running sum", None)):
        a1, a2 = exact.FAMILIES[family]
        M = np.array([[-a1, -a2], [1, 0]], dtype=np.int64)
        for power in (64, 4096):
            P = np.linalg.matrix_power(M, power)
            assert not np.array_equal(P, P.T) and not np.array_equal(P, np.eye(2, dtype=np.int64)), (family, power)
        if period:
            assert np.array_equal(np.linalg.matrix_power(M, period), np.eye(2, dtype=np.int64))
        else:
            assert np.array_equal(np.linalg.matrix_power(M, 4096), [[1, 0], [1, 0]])


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("n", [68, 4100, 8196])
def test_coefficients_of_zero_leave_the_signal(n, causal):
    x = cases.case(n, 1, "resonator", causal)[0][0]
    zero = np.zeros(n, np.float32)
    np.testing.assert_array_equal(emu.tiled_forward(x, zero, zero, causal).view(np.uint32), x.view(np.uint32))
