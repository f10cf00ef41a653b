"""CPU tests of the cascade on frames with a state that enters and leaves the call (rf_var2_plan_execute_cascade_frames_stream):
the serial loop of a chunk pinned against the unchunked loops, the condition the seeds of tests/stream_cases.py are chosen by --
the numpy replay of the chunk chain, forward and backward, at or below half the GPU tests' bar on every output of every case --
the serial adjoint's grad_state_in against central differences, the same replay with the state dropped
far above the bar, and, on a host-only plan, the symbols, the launch counts and names, the byte query and every refusal in the
header's order.  No kernel is launched."""
import ctypes

import numpy as np
import pytest

import cascade_loops
import frames_loops
import recfilter_amd as rfa
import stream_cases as cases
import stream_loops
from recfilter_amd import capi

NEW_SYMBOLS = ["rf_var2_plan_execute_cascade_frames_stream", "rf_var2_plan_execute_cascade_frames_stream_timed",
               "rf_var2_plan_cascade_frames_stream_num_kernels", "rf_var2_plan_cascade_frames_stream_state_bytes",
               "rf_var2_plan_backward_cascade_frames_stream", "rf_var2_plan_backward_cascade_frames_stream_timed",
               "rf_var2_plan_backward_cascade_frames_stream_num_kernels"]
INVALID, UNSUPPORTED, HOST_ONLY = capi.RF_ERR_INVALID_ARG, capi.RF_ERR_UNSUPPORTED, capi.RF_ERR_HIP


def name_of(causal):
    return "causal" if causal else "anticausal"


def host_plan(length, lines=1, causal=True, stride=None):
    return rfa.Var2Plan(length, lines=lines, causal=causal, device=capi.RF_DEVICE_HOST_ONLY, stride=stride)


# ---- the serial loop of a chunk ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", cases.DIRECTIONS)
@pytest.mark.parametrize("hop,chunks,lines,K", [(64, (64, 64, 64), 1, 2), (64, (128, 4), 1, 2), (64, (192, 192, 8), 1, 3), (64, (128, 68), 70, 2)])
def test_chunks_chained_in_f64_are_the_unchunked_loops(hop, chunks, lines, K, causal):
    x, sections, _ = cases.case(hop, chunks, lines, K, "resonator", causal)
    n = sum(chunks)
    whole = [tuple(frames_loops.expand_all(s, hop, n, np.float64)) for s in sections]
    want = cascade_loops.forward(x, whole, causal, np.float64)
    got = [np.empty_like(w) for w in want]
    state = None
    for start, m, first, count in cases.pieces(chunks, hop, causal):
        own = [tuple(frames_loops.expand_all(s, hop, m, np.float64)) for s in cases.chunk_frames(sections, first, count)]
        ys, state = stream_loops.forward(x[:, start:start + m], own, state, causal, np.float64)
        for g, y in zip(got, ys):
            g[:, start:start + m] = y
    for k in range(K):
        peak = float(np.max(np.abs(want[k])))
        assert float(np.max(np.abs(got[k] - want[k]))) <= 1e-12 * peak, f"section {k}"
    # the state that leaves the chain: the two last samples, in the recurrence's order, of x and of every result
    ends = (slice(None), [-1, -2]) if causal else (slice(None), [0, 1])
    for k, signal in enumerate([x.astype(np.float64)] + got):
        assert np.array_equal(state[:, k, :], signal[ends])


@pytest.mark.parametrize("causal", cases.DIRECTIONS)
@pytest.mark.parametrize("hop,chunks,lines,K", [(64, (64, 64, 64), 1, 2), (64, (128, 4), 1, 2), (64, (192, 192, 8), 1, 3)])
def test_adjoints_chained_in_f64_are_the_unchunked_adjoint(hop, chunks, lines, K, causal):
    """the gradients taken through the chain of chunks -- every chunk's grad_state_in handed to the chunk before it -- are
    cascade_loops.adjoint on the whole signal to 1e-12 of the peak; a frame two chunks share sums both pieces"""
    x, sections, g = cases.case(hop, chunks, lines, K, "near one", causal)
    n = sum(chunks)
    whole = [tuple(frames_loops.expand_all(s, hop, n, np.float64)) for s in sections]
    ys = cascade_loops.forward(x, whole, causal, np.float64)
    want_x, want = cascade_loops.adjoint(x, whole, ys, g, causal, np.float64)
    fed, state = [], None
    for start, m, first, count in cases.pieces(chunks, hop, causal):
        own = [tuple(frames_loops.expand_all(s, hop, m, np.float64)) for s in cases.chunk_frames(sections, first, count)]
        results, leaving = stream_loops.forward(x[:, start:start + m], own, state, causal, np.float64)
        fed.append((start, m, own, results, state))
        state = leaving
    got_x, got, gso = np.empty_like(want_x), [[np.zeros_like(p) for p in s] for s in want], None
    for start, m, own, results, entering in fed[::-1]:
        gx, grads, gso = stream_loops.adjoint(x[:, start:start + m], own, results, g[:, start:start + m], entering, gso, causal, np.float64)
        got_x[:, start:start + m] = gx
        for k in range(K):
            for c in range(5):
                got[k][c][:, start:start + m] = grads[k][c]
    assert float(np.max(np.abs(got_x - want_x))) <= 1e-12 * float(np.max(np.abs(want_x)))
    for k in range(K):
        for c in range(5):
            # (per sample the whole signal's gradient has 0 at its masked slots and so has the first chunk's: no state entered it)
            assert float(np.max(np.abs(got[k][c] - want[k][c]))) <= 1e-12 * max(float(np.max(np.abs(want[k][c]))), 1e-30), (k, c)


@pytest.mark.parametrize("causal", cases.DIRECTIONS)
def test_grad_state_in_is_the_central_difference(causal):
    """16 samples, two sections, f64: d(sum(g * out) + sum(G * leaving)) / d(state) by central differences"""
    rng = np.random.default_rng(5)
    n, K = 16, 2
    x, g = rng.standard_normal((1, n)), rng.standard_normal((1, n))
    sections = [tuple(0.4 * rng.standard_normal((1, n)) for _ in range(5)) for _ in range(K)]
    state, G = rng.standard_normal((1, K + 1, 2)), rng.standard_normal((1, K + 1, 2))

    def loss(s):
        ys, leaving = stream_loops.forward(x, sections, s, causal)
        return float(np.sum(g * ys[-1]) + np.sum(G * leaving))
    ys, _ = stream_loops.forward(x, sections, state, causal)
    _, _, got = stream_loops.adjoint(x, sections, ys, g, state, G, causal)
    want, eps = np.empty_like(state), 1e-6
    for at in np.ndindex(*state.shape):
        up, down = state.copy(), state.copy()
        up[at] += eps
        down[at] -= eps
        want[at] = (loss(up) - loss(down)) / (2 * eps)
    # the loss is linear in the state: the difference quotient is exact but for f64 rounding of values of size ~10 over 2e-6
    assert float(np.max(np.abs(got - want))) <= 1e-8 * max(1.0, float(np.max(np.abs(want))))


# ---- the seeds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,chunks,lines,K,kind,causal", cases.UNDER_THE_BAR)
def test_replay_at_or_below_half_the_bar_on_every_gpu_case(hop, chunks, lines, K, kind, causal):
    want = cases.expected(hop, chunks, lines, K, kind, causal)
    got, states = cases.replay(hop, chunks, lines, K, kind, causal)
    for name in cases.names(K):
        cases.assert_under_half_the_bar(got[name], want[name], f"replay hop {hop} {chunks} x {lines} K={K} {kind} {name_of(causal)} {name}")
    got = got["out"]
    ends = (slice(None), [-1, -2]) if causal else (slice(None), [0, 1])      # of the chunk fed last
    start, n = cases.pieces(chunks, hop, causal)[-1][:2]
    x = cases.case(hop, chunks, lines, K, kind, causal)[0]
    assert np.array_equal(states[:, 0], x[:, start:start + n][ends]) and np.array_equal(states[:, K], got[:, start:start + n][ends])


@pytest.mark.parametrize("hop,chunks,lines,K,kind,causal", [c for c in cases.ALL if sum(c[1]) >= 4096])
def test_replay_with_the_state_dropped_is_far_above_the_bar(hop, chunks, lines, K, kind, causal):
    """chunks stitched without the state are wrong, not slightly wrong: at least 100 x the bar on out"""
    reference, err32, peak = cases.expected(hop, chunks, lines, K, kind, causal)["out"]
    got = cases.replay(hop, chunks, lines, K, kind, causal, drop_state=True)[0]["out"]
    err, bar = cases._figure(got, reference, peak), max(4 * err32, 1e-6)
    print(f"state dropped, hop {hop} {chunks} x {lines} K={K} {kind} {name_of(causal)}: err/peak {err:.3e}, {err / bar:.0f} x the bar")
    assert err >= 100 * bar, f"at {err / bar:.1f} x the bar only"


def test_the_cases_without_a_seed_are_those_the_table_names():
    assert len(cases.ALL) == 60 and len(cases.NO_SEED) <= 2 and all(c in cases.ALL and not c[5] for c in cases.NO_SEED)
    assert len(cases.UNDER_THE_BAR) == len(cases.ALL) - len(cases.NO_SEED)
    assert all(key in cases.ALL and 0 < seed < 32 for key, seed in cases.SEEDS.items())


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_front_end():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTED_SYMBOLS and getattr(L, name)
    assert capi.RF_ABI == 3 and b"abi 3" in L.rf_version()
    for name in ("biquad_cascade_frames_stream", "BiquadCascadeStream"):
        assert name in rfa.__all__ and callable(getattr(rfa, name))
    for method in ("execute_cascade_frames_stream", "execute_cascade_frames_stream_timed", "apply_cascade_frames_stream",
                   "cascade_frames_stream_num_kernels", "cascade_frames_stream_state_bytes", "backward_cascade_frames_stream",
                   "backward_cascade_frames_stream_timed", "backward_cascade_frames_stream_num_kernels"):
        assert callable(getattr(rfa.Var2Plan, method))
    assert all(callable(getattr(rfa.BiquadCascadeStream, m)) for m in ("push", "reset"))


def stream_names(K, keep):
    link = "var2_frames_link_keep_stream_1d" if keep else "var2_frames_link_stream_1d"
    return ["var2_biquad_frames_tails_stream_1d"] + ["var2_carry_1d", link] * (K - 1) + ["var2_carry_1d", "var2_frames_pass2_stream_1d"]


def plain_names(K, keep):
    if K == 1:
        return ["var2_biquad_frames_tails_1d", "var2_carry_1d", "var2_frames_pass2_1d"]
    link = "var2_frames_link_keep_1d" if keep else "var2_frames_link_1d"
    return ["var2_biquad_frames_tails_1d"] + ["var2_carry_1d", link] * (K - 1) + ["var2_carry_1d", "var2_frames_pass2_1d"]


def stream_backward_names(K, with_frames):
    last = ["var2_carry_1d", "var2_adj_frames_pass2_stream_1d", "var2_biquad_frames_grad_stream_1d"]
    boundary = (["var2_carry_1d", "var2_adj_frames_link_keep_stream_1d", "var2_frames_coef_stream_1d"] if with_frames
                else ["var2_carry_1d", "var2_adj_frames_link_stream_1d"])
    return ["var2_adj_frames_tails_stream_1d"] + boundary * (K - 1) + last + (["var2_frames_fold_cascade_1d"] if with_frames else [])


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
        assert plan.cascade_frames_stream_num_kernels(K) == len(stream_names(K, False)) == 2 * K + 1
        sections = [None] * K
        for keep in (False, True):
            for state, state_out in ((True, None), (None, None), (True, False)):
                *p, _, _, _, s = plan._cascade_frames_stream_arguments(None, sections, hop, state, None, keep, None, state_out, None)
                got = reported_names(lambda *r: L.rf_var2_plan_execute_cascade_frames_stream_timed(plan._h, *p, s, *r), 2 * K + 1)
                assert got == stream_names(K, keep and K >= 2)
            # both state pointers null: the existing call, its count and its names
            *p, _, _, _, s = plan._cascade_frames_stream_arguments(None, sections, hop, None, None, keep, None, False, None)
            count = plan.cascade_frames_num_kernels(K)
            got = reported_names(lambda *r: L.rf_var2_plan_execute_cascade_frames_stream_timed(plan._h, *p, s, *r), count)
            assert got == plain_names(K, keep)
        for with_frames in (False, True):
            count = 3 * K + 2 if with_frames else 2 * K + 2
            assert plan.backward_cascade_frames_stream_num_kernels(K, with_frames) == len(stream_backward_names(K, with_frames)) == count
            grads = [None] * K if with_frames else None
            for state, gso, gsi in ((True, True, None), (None, True, False), (True, None, False), (None, None, None)):
                *p, _, _, _, s = plan._backward_cascade_frames_stream_arguments(None, sections, hop, None, None, None, None, grads, state, gso, gsi, None)
                got = reported_names(lambda *r: L.rf_var2_plan_backward_cascade_frames_stream_timed(plan._h, *p, s, *r), count)
                assert got == stream_backward_names(K, with_frames)
            # every state pointer null: the existing call, its count and its names
            *p, _, _, _, s = plan._backward_cascade_frames_stream_arguments(None, sections, hop, None, None, None, None, grads, None, None, False, None)
            *q, _, _, t = plan._backward_cascade_frames_arguments(None, sections, hop, None, None, None, None, grads, None)
            count = plan.backward_cascade_frames_num_kernels(K, with_frames)
            assert (reported_names(lambda *r: L.rf_var2_plan_backward_cascade_frames_stream_timed(plan._h, *p, s, *r), count)
                    == reported_names(lambda *r: L.rf_var2_plan_backward_cascade_frames_timed(plan._h, *q, t, *r), count))
        # a report one slot short is refused behind the section count and before everything else
        *p, _, _, _, s = plan._cascade_frames_stream_arguments(None, sections, hop, True, None, False, None, None, None)
        assert L.rf_var2_plan_execute_cascade_frames_stream_timed(plan._h, *p, s, (ctypes.c_float * 64)(), None, 2 * K) == INVALID
        assert b"ms_out" in L.rf_last_error_string()


@pytest.mark.parametrize("length,lines,stride", [(4, 1, 4), (4100, 3, 4112)])
def test_queries_of_host_only_plans(length, lines, stride):
    with host_plan(length, lines, True, stride) as plan:
        for K in (1, 2, 16):
            assert plan.cascade_frames_stream_state_bytes(K) == 4 * lines * 2 * (K + 1)
            assert plan.cascade_frames_stream_state_bytes(K, 40) == 4 * ((lines - 1) * 40 + 2 * (K + 1))
            assert plan.cascade_frames_stream_state_bytes(K, 2 * K + 1) == 0
        for K in (0, 17, -1):
            assert plan.cascade_frames_stream_num_kernels(K) == 0 and plan.cascade_frames_stream_state_bytes(K, 64) == 0
    null, L = ctypes.c_void_p(), capi.lib()
    assert L.rf_var2_plan_cascade_frames_stream_num_kernels(null, 2) == 0 and L.rf_var2_plan_cascade_frames_stream_state_bytes(null, 2, 6) == 0


# ---- the refusals of a call, on addresses that are only numbers ---------------------------------------------------------------------
LENGTH, LINES, STRIDE, HOP = 4100, 3, 4112, 64
COUNT = 66                                    # ceil(4100 / 64) + 1
FSTRIDE = COUNT + 2
K = 3
SSTRIDE = 2 * (K + 1) + 4
A = [(i + 1) << 20 for i in range(64)]
X, OUT, SIN, SOUT = A[:4]
KEPT = A[4:6]
FRAMES = [A[8 + 5 * k:13 + 5 * k] for k in range(K)]            # A[8] .. A[22]


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


def raw_stream(a):
    with host_plan(LENGTH, LINES, True, STRIDE) as plan:
        status = capi.lib().rf_var2_plan_execute_cascade_frames_stream(
            plan._h, ctypes.c_void_p(a["x"]), sections_of(a["frames"]), a["K"], a["hop"], a["count"], a["fstride"], ctypes.c_void_p(a["out"]),
            pointers(a["kept"]), ctypes.c_void_p(a["sin"]), ctypes.c_void_p(a["sout"]), a["sstride"], None)
        return status, capi.lib().rf_last_error_string().decode()


E = dict(x=X, frames=FRAMES, K=K, hop=HOP, count=COUNT, fstride=FSTRIDE, out=OUT, kept=None, sin=SIN, sout=SOUT, sstride=SSTRIDE)
EK = put(E, kept=KEPT)


@pytest.mark.parametrize("what,a,status,text", [
    ("valid: only the host-only refusal is left", E, HOST_ONLY, "host-only"),
    ("valid, keeping", EK, HOST_ONLY, "host-only"),
    ("valid, no state enters", put(E, sin=0), HOST_ONLY, "host-only"),
    ("valid, no state wanted", put(E, sout=0), HOST_ONLY, "host-only"),
    ("valid, no state at all: the existing call", put(E, sin=0, sout=0, sstride=0), HOST_ONLY, "host-only"),
    ("valid, one section", put(E, K=1), HOST_ONLY, "host-only"),
    ("valid, the smallest stride", put(E, sstride=2 * (K + 1)), HOST_ONLY, "host-only"),
    ("valid, state_in is in (both are read)", put(E, sin=X), HOST_ONLY, "host-only"),
    *[(f"{k} sections", put(E, K=k), INVALID, "n_sections must be") for k in (0, -1, 17)],
    ("hop 480", put(E, hop=480), UNSUPPORTED, "power of two"),
    ("a frame short", put(E, count=COUNT - 1), INVALID, "n_frames must be"),
    ("frame stride below the count", put(E, fstride=COUNT - 1), INVALID, "frame_stride"),
    ("null frames", put(E, frames=None), INVALID, "null"),
    ("null in", put(E, x=0), INVALID, "null"),
    ("in 4 bytes off", put(E, x=X + 4), INVALID, "aligned"),
    ("in == out", put(E, out=X), INVALID, "in == out is not allowed"),
    ("the kept signals overlap", put(EK, kept=[KEPT[0], KEPT[0] + 16]), INVALID, "kept plane 0 overlaps kept plane 1"),
    ("a state stride one short", put(E, sstride=2 * (K + 1) - 1), INVALID, "state_stride"),
    ("a state stride of 0", put(E, sstride=0), INVALID, "state_stride"),
    ("state_in 2 bytes off", put(E, sin=SIN + 2), INVALID, "state buffers need 4-byte aligned"),
    ("state_out 1 byte off", put(E, sout=SOUT + 1), INVALID, "state buffers need 4-byte aligned"),
    ("state_in 4 bytes off is fine", put(E, sin=SIN + 4), HOST_ONLY, "host-only"),
    ("state_out is state_in", put(E, sout=SIN), INVALID, "state_out overlaps state_in"),
    ("state_out overlaps the last line of state_in", put(E, sout=SIN + 4 * (2 * SSTRIDE + 7)), INVALID, "state_out overlaps state_in"),
    ("state_out just behind state_in", put(E, sout=SIN + 4 * (2 * SSTRIDE + 8)), HOST_ONLY, "host-only"),
    ("state_out is in", put(E, sout=X), INVALID, "state_out overlaps in"),
    ("state_out in the last line of out", put(E, sout=OUT + 4 * (2 * STRIDE + LENGTH - 1)), INVALID, "state_out overlaps out"),
    ("state_out is a kept signal", put(EK, sout=KEPT[1]), INVALID, "state_out overlaps kept plane 1"),
    ("state_out is a frame array", put(E, sout=FRAMES[2][3]), INVALID, "state_out overlaps frames of section 2 plane 3"),
    ("state_in is out", put(E, sin=OUT), INVALID, "state_in overlaps out"),
    ("state_in is a kept signal", put(EK, sin=KEPT[0]), INVALID, "state_in overlaps kept plane 0"),
    # the header's order: the existing call's refusals, the state's stride, its alignment, its overlaps
    ("the section count before the state", put(E, K=0, sstride=0), INVALID, "n_sections must be"),
    ("an overlap of out before the state's stride", put(E, out=X, sstride=0), INVALID, "in == out"),
    ("a kept overlap before the state's stride", put(EK, kept=[X, KEPT[1]], sstride=0), INVALID, "kept plane 0 overlaps in"),
    ("the stride before the alignment", put(E, sstride=1, sin=SIN + 2), INVALID, "state_stride"),
    ("alignment before overlap", put(E, sin=SIN + 2, sout=SIN), INVALID, "aligned"),
    ("state_out's overlaps before state_in's", put(E, sin=OUT, sout=X), INVALID, "state_out overlaps in"),
])
def test_execute_cascade_frames_stream_refusals(what, a, status, text):
    got, message = raw_stream(a)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"


GOUT, GIN, GSO, GSI = A[40:44]
GRADS = [A[24 + 5 * k:29 + 5 * k] for k in range(K)]            # A[24] .. A[38]


def raw_stream_backward(a):
    with host_plan(LENGTH, LINES, True, STRIDE) as plan:
        status = capi.lib().rf_var2_plan_backward_cascade_frames_stream(
            plan._h, ctypes.c_void_p(a["x"]), sections_of(a["frames"]), a["K"], a["hop"], a["count"], a["fstride"], pointers(a["kept"]),
            ctypes.c_void_p(a["out"]), ctypes.c_void_p(a["gout"]), ctypes.c_void_p(a["gin"]), sections_of(a["grads"]), ctypes.c_void_p(a["sin"]),
            ctypes.c_void_p(a["gso"]), ctypes.c_void_p(a["gsi"]), a["sstride"], None)
        return status, capi.lib().rf_last_error_string().decode()


B = dict(EK, gout=GOUT, gin=GIN, grads=GRADS, gso=GSO, gsi=GSI)
del B["sout"]


@pytest.mark.parametrize("what,a,status,text", [
    ("valid, with frame gradients", B, HOST_ONLY, "host-only"),
    ("valid, nothing of the forward", put(B, grads=None, x=0, out=0, kept=None, sin=0), HOST_ONLY, "host-only"),
    ("valid, no gradient of the leaving state", put(B, gso=0), HOST_ONLY, "host-only"),
    ("valid, no gradient of the entering state wanted", put(B, gsi=0), HOST_ONLY, "host-only"),
    ("valid, no state at all: the existing call", put(B, sin=0, gso=0, gsi=0, sstride=0), HOST_ONLY, "host-only"),
    ("valid, one section", put(B, K=1), HOST_ONLY, "host-only"),
    ("valid, grad_in is grad_out", put(B, gin=GOUT), HOST_ONLY, "host-only"),
    ("17 sections", put(B, K=17), INVALID, "n_sections must be"),
    ("hop 480", put(B, hop=480), UNSUPPORTED, "power of two"),
    ("null grad_out", put(B, gout=0), INVALID, "null"),
    ("frame gradients without kept", put(B, kept=None), INVALID, "kept 0"),
    ("grad_in is in", put(B, gin=X), INVALID, "grad_in plane 0 overlaps in"),
    ("a state stride one short", put(B, sstride=2 * (K + 1) - 1), INVALID, "state_stride"),
    *[(f"{k} 2 bytes off", put(B, **{k: B[k] + 2}), INVALID, "state buffers need 4-byte aligned") for k in ("sin", "gso", "gsi")],
    ("grad_state_in is state_in", put(B, gsi=SIN), INVALID, "grad_state_in overlaps state_in"),
    ("grad_state_in is grad_state_out", put(B, gsi=GSO), INVALID, "grad_state_in overlaps grad_state_out"),
    ("grad_state_in is grad_out", put(B, gsi=GOUT), INVALID, "grad_state_in overlaps grad_out"),
    ("grad_state_in is grad_in", put(B, gsi=GIN), INVALID, "grad_state_in overlaps grad_in"),
    ("grad_state_in is a kept signal", put(B, gsi=KEPT[1]), INVALID, "grad_state_in overlaps kept plane 1"),
    ("grad_state_in is a frame array", put(B, gsi=FRAMES[1][2]), INVALID, "grad_state_in overlaps frames of section 1 plane 2"),
    ("grad_state_in is a frame gradient", put(B, gsi=GRADS[2][4]), INVALID, "grad_state_in overlaps gradient of frames of section 2 plane 4"),
    ("the stride before the alignment", put(B, sstride=1, gso=GSO + 2), INVALID, "state_stride"),
    ("an overlap of grad_in before the state", put(B, gin=X, sstride=0), INVALID, "grad_in plane 0 overlaps in"),
])
def test_backward_cascade_frames_stream_refusals(what, a, status, text):
    got, message = raw_stream_backward(a)
    assert got == status, f"{what}: status {got} ({message})"
    assert message and text in message, f"{what}: {message!r}"


def test_null_plan_is_refused():
    null, L = ctypes.c_void_p(), capi.lib()
    assert L.rf_var2_plan_execute_cascade_frames_stream(null, null, None, 2, 64, 66, 66, null, None, null, null, 6, null) == INVALID
    assert L.rf_last_error_string()


def test_the_functional_form_refuses_a_ragged_chunk():
    torch = pytest.importorskip("torch")
    frames = [tuple(torch.zeros(2) for _ in range(5))]
    for n in (6, 2, 0):
        with pytest.raises(ValueError, match="multiple of 4"):
            rfa.biquad_cascade_frames_stream(torch.zeros(n), frames, 64)
    with pytest.raises(ValueError, match="sections"):
        rfa.biquad_cascade_frames_stream(torch.zeros(8), [], 64)
    with pytest.raises(ValueError, match="sections"):
        rfa.BiquadCascadeStream(0, 64)
    with pytest.raises(ValueError):
        rfa.BiquadCascadeStream(2, 480)
