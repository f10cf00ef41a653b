"""GPU tests of the cascade on frames with a state that enters and leaves the call (rf_var2_plan_execute_cascade_frames_stream: the
STREAM instances of var2_frames_kernel and var2_frames_link_kernel of kernels_var2_signal.hip, plan_var2.cpp,
Var2Plan.execute_cascade_frames_stream / biquad_cascade_frames_stream / BiquadCascadeStream of recfilter_amd/var2.py).

The pins are the call without a state.  No state, or a state of zeros, is execute_cascade_frames; with one section and b = (1, 0, 0)
the call with a feedback history is execute_cascade_frames on an input whose two first samples the host has modified with fma; with
all feedback frames 0 the two first results are the host's fma values and the rest the call without a state, bit for bit.  The state
that leaves is the two last samples of x, of every kept signal and of out.  End to end a signal filtered in chunks is under the
family's bar against the f64 loops on the WHOLE signal, forward and -- through rf_var2_plan_backward_cascade_frames_stream, the
gradients handed from chunk to chunk -- grad_x, the 5 K frame gradients and grad_state_in; cases, seeds and bar: tests/stream_cases.py (tests/test_stream_host.py holds
the numpy replay at half the bar on every case here)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import frames_loops as loops
import recfilter_amd as rfa
import stream_cases as cases
import var2_emulator as emu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = cases.DIRECTIONS
F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def name_of(causal):
    return "causal" if causal else "anticausal"


def device_lines(a, stride=None):
    """an (L, N) array on the device: (N,) for one line, else rows `stride` apart (NaN between them)"""
    import torch
    a = np.asarray(a)
    lines, n = a.shape
    if lines == 1:
        return torch.from_numpy(np.array(a[0])).cuda()
    wide = torch.full((lines, stride or n), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :n] = torch.from_numpy(np.array(a)).cuda()
    return wide[:, :n]


def device_sections(sections):
    """every frame array on the device, rows F + FRAME_PAD apart where there are lines"""
    return [tuple(device_lines(f, np.asarray(f).shape[1] + cases.FRAME_PAD) for f in s) for s in sections]


def device_state(a):
    """a (L, K + 1, 2) state on the device: (K + 1, 2) for one line"""
    import torch
    a = np.asarray(a, dtype=F)
    return torch.from_numpy(np.array(a[0] if a.shape[0] == 1 else a)).cuda()


def host(t, lines):
    return t.cpu().numpy().reshape(lines, -1)


def ends(a, causal):
    """the two last samples of (L, n) in the order of the recurrence: (L, 2)"""
    return a[:, [-1, -2]] if causal else a[:, [0, 1]]


def chain(x, sections, hop, chunks, lines, causal, stride, keep, g=None):
    """the chunks of one case through execute_cascade_frames_stream, every chunk addressed in place in the whole signal's arrays;
    ([out], [kept k], [(the chunk's first sample, its length, the state that left it)], nothing between the lines) on the host.
    g (keeping): then backward_cascade_frames_stream from the chunk fed last back to the first, each chunk's grad_state_in handed
    to the chunk before it; a fifth element, ({name: array} of cases.names(K) but "out", twice: with and without frame gradients)"""
    import torch
    n, K = sum(chunks), len(sections)
    dx, ds = device_lines(x, stride), device_sections(sections)
    fresh = lambda: device_lines(np.full((lines, n), np.nan, F), stride)      # noqa: E731
    out, kept = fresh(), [fresh() for _ in range(K - 1)] if keep else None
    state, states = None, []
    plans = {}
    try:
        for start, m, first, count in cases.pieces(chunks, hop, causal):
            if m not in plans:
                plans[m] = rfa.Var2Plan(m, lines=lines, causal=causal, stride=(stride or n) if lines > 1 else None)
            own = cases.chunk_frames(ds, first, count)
            at = (Ellipsis, slice(start, start + m))
            if keep:
                _, _, state = plans[m].execute_cascade_frames_stream(dx[at], own, hop, state, out[at], kept=[t[at] for t in kept])
            else:
                _, state = plans[m].execute_cascade_frames_stream(dx[at], own, hop, state, out[at])
            states.append((start, m, state))
        torch.cuda.synchronize()
        backward = None
        if g is not None:
            dg, count = device_lines(g, stride), loops.frames_count(n, hop)
            backward = []
            for with_frames in (True, False):
                gin, gso, per_chunk = fresh(), None, []
                fed = cases.pieces(chunks, hop, causal)
                for i in range(len(fed) - 1, -1, -1):
                    start, m, first, frames = fed[i]
                    at = (Ellipsis, slice(start, start + m))
                    own = cases.chunk_frames(ds, first, frames)
                    # (laid out like the chunk's frames: rows as far apart as the whole signal's)
                    grads = [tuple(device_lines(np.full((lines, frames), np.nan, F), ds[0][0].stride(0) if lines > 1 else None) for _ in range(5))
                             for _ in range(K)]
                    entering = states[i - 1][2] if i > 0 else None
                    if with_frames:
                        _, grads, gso = plans[m].backward_cascade_frames_stream(dx[at], own, hop, [t[at] for t in kept], out[at], dg[at], gin[at], grads,
                                                                                entering, gso)
                    else:      # nothing of the forward is handed in
                        _, _, gso = plans[m].backward_cascade_frames_stream(None, own, hop, None, None, dg[at], gin[at], None, None, gso)
                        grads = []
                    per_chunk.append((start, m, first, frames, host(out[at], lines), host(gin[at], lines), [host(t, lines) for s in grads for t in s]))
                torch.cuda.synchronize()
                got = cases.gather(K if with_frames else 0, lines, n, count, per_chunk)
                got["grad_state_in"] = gso.cpu().numpy().reshape(lines, K + 1, 2)
                got["between the lines"] = bool(torch.isnan(gin._base[:, n:]).all()) if lines > 1 else True
                backward.append(got)
    finally:
        for plan in plans.values():
            plan.close()
    between = all(bool(torch.isnan(t._base[:, n:]).all()) for t in [out] + (kept or [])) if lines > 1 else True
    result = (host(out, lines), [host(t, lines) for t in kept or []], [(s, m, t.cpu().numpy().reshape(lines, K + 1, 2)) for s, m, t in states], between)
    return result + ((backward,) if g is not None else ())


@functools.lru_cache(maxsize=None)
def run(hop, chunks, lines, K, kind, causal):
    """the chains of one case, once: plain, again, and keeping; shared by the tests below and never written"""
    x, sections, g = cases.case(hop, chunks, lines, K, kind, causal)
    stride = cases.STRIDES.get((lines, sum(chunks)))
    r = {name: chain(x, sections, hop, chunks, lines, causal, stride, keep) for name, keep in (("plain", False), ("again", False))}
    r["keep"] = chain(x, sections, hop, chunks, lines, causal, stride, True, g)
    r["keep again"] = chain(x, sections, hop, chunks, lines, causal, stride, True, g)
    return r


# ---- 1: no state, or a state of zeros -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("hop,chunks,lines,K", [(64, (64, 64, 64), 1, 2), (64, (4160, 4160), 1, 1), (64, (192, 192, 8), 1, 3), (64, (128, 68), 70, 2)])
def test_no_state_and_a_state_of_zeros_are_the_call_without_one(hop, chunks, lines, K, causal):
    import torch
    x, sections, _ = cases.case(hop, chunks, lines, K, "resonator", causal)
    n = chunks[0]
    stride = cases.STRIDES.get((lines, sum(chunks))) if lines > 1 else None
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        dx = device_lines(x, stride)[..., :n]
        ds = cases.chunk_frames(device_sections(sections), 0, loops.frames_count(n, hop))
        want, want_kept = plan.execute_cascade_frames(dx, ds, hop, keep=True)
        both_null, none = plan.execute_cascade_frames_stream(dx, ds, hop, None, state_out=False)
        assert none is None
        _, both_null_times = plan.execute_cascade_frames_stream_timed(dx, ds, hop, None, state_out=False)[::2]
        _, plain_times = plan.execute_cascade_frames_timed(dx, ds, hop)
        no_entry, kept, left = plan.execute_cascade_frames_stream(dx, ds, hop, None, keep=True)
        zeros = device_state(np.zeros((lines, K + 1, 2), F))
        from_zeros, left_from_zeros, stream_times = plan.execute_cascade_frames_stream_timed(dx, ds, hop, zeros)
        only_in, none = plan.execute_cascade_frames_stream(dx, ds, hop, zeros, state_out=False)
        torch.cuda.synchronize()
        assert none is None
    assert [name for name, _ in both_null_times] == [name for name, _ in plain_times]      # the existing call, its launches
    assert len(stream_times) == 2 * K + 1 and all(name.endswith("_stream_1d") or name == "var2_carry_1d" for name, _ in stream_times)
    np.testing.assert_array_equal(bits(host(both_null, lines)), bits(host(want, lines)))
    np.testing.assert_array_equal(bits(host(no_entry, lines)), bits(host(want, lines)))      # nothing is folded where nothing enters
    for k in range(K - 1):
        np.testing.assert_array_equal(bits(host(kept[k], lines)), bits(host(want_kept[k], lines)), f"kept {k}")
    assert np.array_equal(host(from_zeros, lines), host(want, lines))      # (a zero's sign apart)
    np.testing.assert_array_equal(bits(host(only_in, lines)), bits(host(from_zeros, lines)))
    np.testing.assert_array_equal(bits(host(left, lines)), bits(host(left_from_zeros, lines)))


# ---- 2: the feedback history -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("n", [4, 68, 4160])
def test_feedback_history_is_the_call_on_an_input_modified_in_two_samples(n, kind, causal):
    """K = 1, b = (1, 0, 0): the call with (hy1, hy2) is execute_cascade_frames on x', x'[0] = fma(-a1[0], hy1, fma(-a2[0], hy2, x[0]))
    and x'[1] = fma(-a2[1], hy1, x[1]) formed on the host (an anticausal plan: samples n - 1 and n - 2); the input's history
    meets taps of 0"""
    import torch
    hop = 64
    x, sections, _ = cases.case(hop, (4160, 4160), 1, 1, kind, causal)
    count = loops.frames_count(n, hop)
    x = x[:, :n]
    a1, a2 = (np.ascontiguousarray(f[:, :count]) for f in sections[0][3:])
    one, zero = np.ones_like(a1), np.zeros_like(a1)
    state = np.array([[[0.75, -0.5], [0.625, -1.375]]], F)
    (hy1, hy2), i0, i1 = state[0, 1], (0 if causal else n - 1), (1 if causal else n - 2)
    e1, e2 = loops.expand(a1[0], hop, n, F), loops.expand(a2[0], hop, n, F)
    modified = x.copy()
    modified[0, i0] = emu.fma(-e1[i0], hy1, emu.fma(-e2[i0], hy2, x[0, i0]))
    modified[0, i1] = emu.fma(-e2[i1], hy1, x[0, i1])
    with rfa.Var2Plan(n, causal=causal) as plan:
        ds = device_sections([(one, zero, zero, a1, a2)])
        got, left = plan.execute_cascade_frames_stream(device_lines(x), ds, hop, device_state(state))
        want = plan.execute_cascade_frames(device_lines(modified), ds, hop)
        torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(host(got, 1)), bits(host(want, 1)))
    np.testing.assert_array_equal(bits(host(left, 1)), bits(np.concatenate([ends(x, causal), ends(host(got, 1), causal)], axis=1)))


# ---- 3: the input's history ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("n", [4, 68, 4160])
def test_input_history_reaches_the_two_first_results_alone(n, causal):
    """all feedback frames 0: out[0] = fma(b2[0], hx2, fma(b1[0], hx1, b0[0] x[0])) and out[1] = fma(b2[1], hx1, fma(b1[1], x[0],
    b0[1] x[1])), the host's values, and out[2:] is the call without a state; the result's history meets feedback of 0"""
    import torch
    hop = 64
    x, sections, _ = cases.case(hop, (4160, 4160), 1, 1, "resonator", causal)
    count = loops.frames_count(n, hop)
    x = x[:, :n]
    b0, b1, b2 = (np.ascontiguousarray(f[:, :count]) for f in sections[0][:3])
    zero = np.zeros_like(b0)
    state = np.array([[[0.75, -0.5], [0.625, -1.375]]], F)
    (hx1, hx2), i0, i1 = state[0, 0], (0 if causal else n - 1), (1 if causal else n - 2)
    e0, e1, e2 = (loops.expand(b[0], hop, n, F) for b in (b0, b1, b2))
    with rfa.Var2Plan(n, causal=causal) as plan:
        ds = device_sections([(b0, b1, b2, zero, zero)])
        got, _ = plan.execute_cascade_frames_stream(device_lines(x), ds, hop, device_state(state))
        want = host(plan.execute_cascade_frames(device_lines(x), ds, hop), 1)
        torch.cuda.synchronize()
    want[0, i0] = emu.fma(e2[i0], hx2, emu.fma(e1[i0], hx1, e0[i0] * x[0, i0]))
    want[0, i1] = emu.fma(e2[i1], hx1, emu.fma(e1[i1], x[0, i0], e0[i1] * x[0, i1]))
    np.testing.assert_array_equal(bits(host(got, 1)), bits(want))


# ---- 4: the state that leaves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,chunks,lines,K,kind,causal", cases.ALL)
def test_leaving_state_is_the_last_two_samples_of_every_signal(hop, chunks, lines, K, kind, causal):
    x = cases.case(hop, chunks, lines, K, kind, causal)[0]
    r = run(hop, chunks, lines, K, kind, causal)
    out, kept, states, between = r["keep"][:4]
    plain, _, plain_states, plain_between = r["plain"]
    assert between and plain_between and not np.isnan(out).any()
    np.testing.assert_array_equal(bits(out), bits(plain))      # keeping or not
    for (start, m, state), (_, _, plain_state) in zip(states, plain_states):
        at = slice(start, start + m)
        for k, signal in enumerate([x] + kept + [out]):
            np.testing.assert_array_equal(bits(state[:, k]), bits(ends(signal[:, at], causal)), f"chunk at {start}: pair {k}")
        np.testing.assert_array_equal(bits(state), bits(plain_state))


# ---- 5: end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,chunks,lines,K,kind,causal", cases.UNDER_THE_BAR)
def test_chunk_chain_is_under_the_bar_of_the_whole_signal(hop, chunks, lines, K, kind, causal):
    want = cases.expected(hop, chunks, lines, K, kind, causal)
    out = run(hop, chunks, lines, K, kind, causal)["plain"][0]
    cases.assert_under_bar(out, want["out"], f"chunks hop {hop} {chunks} x {lines} K={K} {kind} {name_of(causal)} out")


@pytest.mark.parametrize("hop,chunks,lines,K,kind,causal", cases.UNDER_THE_BAR)
def test_gradients_through_the_chunk_chain_are_under_the_bar_of_the_whole_signal(hop, chunks, lines, K, kind, causal):
    """grad_x and the 5 K frame gradients against the f64 loops on the WHOLE signal -- a frame two chunks share sums both pieces --
    and grad_state_in of the chunk fed first against tests/stream_loops.py chained"""
    want = cases.expected(hop, chunks, lines, K, kind, causal)
    with_frames, only_x = run(hop, chunks, lines, K, kind, causal)["keep"][4]
    assert with_frames["between the lines"] and only_x["between the lines"]
    for name in cases.names(K)[1:]:
        cases.assert_under_bar(with_frames[name], want[name], f"chunks hop {hop} {chunks} x {lines} K={K} {kind} {name_of(causal)} {name}")
    # without frame gradients nothing of the forward was handed in: the same grad_x and grad_state_in
    np.testing.assert_array_equal(bits(only_x["grad_x"]), bits(with_frames["grad_x"]))
    np.testing.assert_array_equal(bits(only_x["grad_state_in"]), bits(with_frames["grad_state_in"]))


@pytest.mark.parametrize("hop,chunks,lines,K,kind,causal", cases.ALL)
def test_two_runs_give_the_same_bits(hop, chunks, lines, K, kind, causal):
    r = run(hop, chunks, lines, K, kind, causal)
    np.testing.assert_array_equal(bits(r["plain"][0]), bits(r["again"][0]))
    for (_, _, a), (_, _, b) in zip(r["plain"][2], r["again"][2]):
        np.testing.assert_array_equal(bits(a), bits(b))
    for a, b in zip(r["keep"][4], r["keep again"][4]):
        for name in a:
            np.testing.assert_array_equal(np.asarray(a[name]), np.asarray(b[name]), name)
            assert not np.isnan(np.asarray(a[name], dtype=np.float64)).any(), name


# ---- 5b: the backward without a state, and from zeros -----------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("hop,chunks,lines,K", [(64, (64, 64, 64), 1, 2), (64, (4160, 4160), 1, 1), (64, (192, 192, 8), 1, 3), (64, (128, 68), 70, 2)])
def test_backward_without_a_state_and_from_zeros_is_the_backward_without_one(hop, chunks, lines, K, causal):
    import torch
    x, sections, g = cases.case(hop, chunks, lines, K, "resonator", causal)
    n = chunks[0]
    count = loops.frames_count(n, hop)
    stride = cases.STRIDES.get((lines, sum(chunks))) if lines > 1 else None
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        dx, dg = device_lines(x, stride)[..., :n], device_lines(g, stride)[..., :n]
        ds = cases.chunk_frames(device_sections(sections), 0, count)
        apart = ds[0][0].stride(0) if lines > 1 else None      # the gradients are laid out like the chunk's frames
        fresh = lambda: [tuple(device_lines(np.full((lines, count), np.nan, F), apart) for _ in range(5)) for _ in range(K)]      # noqa: E731
        out, kept = plan.execute_cascade_frames(dx, ds, hop, keep=True)
        want_x, want = plan.backward_cascade_frames(dx, ds, hop, kept, out, dg, None, fresh())
        null_x, null, none, null_times = plan.backward_cascade_frames_stream_timed(dx, ds, hop, kept, out, dg, None, fresh(), None, None, False)
        *_, plain_times = plan.backward_cascade_frames_timed(dx, ds, hop, kept, out, dg, None, fresh())
        zeros = device_state(np.zeros((lines, K + 1, 2), F))
        zero_x, zero, gsi, stream_times = plan.backward_cascade_frames_stream_timed(dx, ds, hop, kept, out, dg, None, fresh(), zeros, zeros.clone())
        only_x, _, gsi_alone = plan.backward_cascade_frames_stream(None, ds, hop, None, None, dg)
        torch.cuda.synchronize()
    assert none is None and [name for name, _ in null_times] == [name for name, _ in plain_times]
    assert len(stream_times) == 3 * K + 2 and sum(name.endswith("_stream_1d") for name, _ in stream_times) == 2 * K + 1
    np.testing.assert_array_equal(bits(host(null_x, lines)), bits(host(want_x, lines)))
    assert np.array_equal(host(zero_x, lines), host(want_x, lines)) and np.array_equal(host(only_x, lines), host(want_x, lines))
    for a, b, c in zip((t for s in want for t in s), (t for s in null for t in s), (t for s in zero for t in s)):
        np.testing.assert_array_equal(bits(host(a, lines)), bits(host(b, lines)))
        assert np.array_equal(host(a, lines), host(c, lines))      # (a zero's sign apart: the history's products are +-0)
    np.testing.assert_array_equal(bits(host(gsi, lines)), bits(host(gsi_alone, lines)))


# ---- 6: the front-ends ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("hop,chunks,lines,K", [(64, (128, 4), 1, 2), (64, (4096, 4160, 68), 1, 2), (64, (128, 68), 70, 2)])
def test_push_is_the_functional_chain_and_the_plan_calls_bit_for_bit(hop, chunks, lines, K, causal):
    import torch
    kind = "near one"
    x, sections, _ = cases.case(hop, chunks, lines, K, kind, causal)
    dx = torch.from_numpy(np.array(x[0] if lines == 1 else x)).cuda()
    ds = [tuple(torch.from_numpy(np.array(f[0] if lines == 1 else f)).cuda() for f in s) for s in sections]
    stream = rfa.BiquadCascadeStream(K, hop, lines=lines, causal=causal)
    pushed, chained = torch.empty_like(dx), torch.empty_like(dx)
    for _ in range(2):      # the second round behind a reset
        state = None
        for start, m, first, count in cases.pieces(chunks, hop, causal):
            at = (Ellipsis, slice(start, start + m))
            own = cases.chunk_frames(ds, first, count)
            pushed[at] = stream.push(dx[at], own)
            chained[at], state = rfa.biquad_cascade_frames_stream(dx[at], own, hop, state, causal=causal)
            assert tuple(state.shape) == tuple(dx.shape[:-1]) + (K + 1, 2)
            np.testing.assert_array_equal(bits(stream.state.cpu().numpy()), bits(state.cpu().numpy()))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(host(pushed, lines)), bits(host(chained, lines)))
        np.testing.assert_array_equal(bits(host(chained, lines)), bits(run(hop, chunks, lines, K, kind, causal)["plain"][0]))
        stream.reset()
        assert stream.state is None
    with pytest.raises(ValueError, match="multiple of 4"):
        rfa.biquad_cascade_frames_stream(dx[..., :6], cases.chunk_frames(ds, 0, 2), hop)


# ---- 6b: autograd through a chain of chunks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("hop,chunks,lines,K", [(64, (128, 4), 1, 2), (64, (192, 192, 8), 1, 3), (64, (128, 68), 70, 2)])
def test_autograd_through_the_functional_chain(hop, chunks, lines, K, causal):
    """a loss on the concatenated results reaches x, every frame tensor and the state of the first chunk through the states between
    the chunks: under the bar against the whole signal's f64 loops; detached states cut the chain (truncated back-propagation)"""
    import torch
    kind = "near one"
    x, sections, g = cases.case(hop, chunks, lines, K, kind, causal)
    want = cases.expected(hop, chunks, lines, K, kind, causal)
    on = lambda a: torch.from_numpy(np.array(a[0] if lines == 1 else a)).cuda()      # noqa: E731
    dx, dg = on(x).requires_grad_(True), on(g)
    ds = [tuple(on(f).requires_grad_(True) for f in s) for s in sections]
    state0 = torch.zeros(((K + 1, 2) if lines == 1 else (lines, K + 1, 2)), device="cuda", requires_grad=True)
    for detach in (False, True):
        for t in [dx, state0] + [f for s in ds for f in s]:
            t.grad = None
        state, loss = state0, 0.0
        for start, m, first, count in cases.pieces(chunks, hop, causal):
            at = (Ellipsis, slice(start, start + m))
            y, state = rfa.biquad_cascade_frames_stream(dx[at], cases.chunk_frames(ds, first, count), hop, state, causal=causal)
            loss = loss + (y * dg[at]).sum()
            if detach:
                state = state.detach()
        loss.backward()
        torch.cuda.synchronize()
        got = {"grad_x": host(dx.grad, lines), "grad_state_in": state0.grad.cpu().numpy().reshape(lines, K + 1, 2)}
        for name, t in zip(cases.names(K)[2:], (f for s in ds for f in s)):
            got[name] = host(t.grad, lines)
        if not detach:
            for name in cases.names(K)[1:]:
                cases.assert_under_bar(got[name], want[name], f"autograd hop {hop} {chunks} x {lines} K={K} {name_of(causal)} {name}")
            full = got
        else:      # only the chunk fed first reaches its state; the last chunk's grad_x is untouched by the cut
            start, m = cases.pieces(chunks, hop, causal)[-1][:2]
            np.testing.assert_array_equal(bits(got["grad_x"][:, start:start + m]), bits(full["grad_x"][:, start:start + m]))
            assert not np.array_equal(got["grad_x"], full["grad_x"])


# ---- 7: the C++ front-end ---------------------------------------------------------------------------------------------------------------
def test_cpp_frontend_cascade_frames_stream(tmp_path):
    """RecFilterVarying2::realize_cascade_frames_stream on a signal of 8384 samples in two chunks, three sections, both directions,
    against the C calls bit for bit; compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_cascade_frames_stream.cpp")
    exe = str(tmp_path / "test_frontend_cascade_frames_stream")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "cascade-frames-stream-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
