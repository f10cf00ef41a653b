"""GPU tests of cascades on control-rate frames (rf_var2_plan_execute_cascade_frames / _backward_cascade_frames:
var2_frames_link_kernel, var2_adj_frames_link_kernel, the COEF_ONLY instances of var2_frames_grad_kernel and
var2_frames_fold_cascade_kernel of kernels_var2_signal.hip, plan_var2.cpp, Var2Plan.execute_cascade_frames / biquad_cascade_frames
of recfilter_amd/var2.py).

The pins are the calls this one fuses.  On the expand_frames signals the forward is execute_cascade BIT FOR BIT -- keeping or not,
and the kept signals are execute_cascade_keep's -- and grad_in is backward_cascade_kept's; one section is execute_biquad_frames /
backward_biquad_frames, launches and bits; with all feedback frames 0 the result is K chained execute_biquad_frames calls.  The
frame gradients are the per-sample gradients backward_cascade_kept stores, contracted: against their f64 contraction they meet the
bound of one rounding to f32 and 2^-36 of the absolute sum.  End to end everything is under the family's bar against the f64
loops; cases, seeds and bar: tests/cascade_frames_cases.py (tests/test_cascade_frames_host.py holds the numpy replay at half the
bar on every case here).  With RECFILTER_PROFILE_DIR set, the worst shares and ratios are written there (profiles/r34)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cascade_frames_cases as cases
import frames_loops as loops
import recfilter_amd as rfa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = cases.DIRECTIONS
SHARES, RATIOS = {}, {}      # case -> the worst |got - s| / bound; case -> the worst err / bar


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


def device_frames(a):
    """an (L, F) frame array on the device: (F,) for one line, else rows F + FRAME_PAD apart (NaN between them)"""
    return device_lines(a, np.asarray(a).shape[1] + cases.FRAME_PAD)


def device_sections(sections):
    return [tuple(device_frames(f) for f in s) for s in sections]


def host(t, lines):
    return t.cpu().numpy().reshape(lines, -1)


def nan_lines(lines, n, stride):
    return device_lines(np.full((lines, n), np.nan, np.float32), stride)


def nan_grads(lines, count, K):
    return [tuple(device_frames(np.full((lines, count), np.nan, np.float32)) for _ in range(5)) for _ in range(K)]


def write_profile(name, rows):
    """<RECFILTER_PROFILE_DIR>/<name> where that variable names a directory (profiles/r34 holds a copy): rewritten behind every
    case with what this process has seen so far, so a selection of cases leaves its own; a pytest-xdist worker writes a file of
    its own"""
    where = os.environ.get("RECFILTER_PROFILE_DIR")
    if where:
        os.makedirs(where, exist_ok=True)
        worker = os.environ.get("PYTEST_XDIST_WORKER")
        with open(os.path.join(where, name if not worker else f"{worker}.{name}"), "w") as f:
            f.writelines(rows)


@functools.lru_cache(maxsize=None)
def run(hop, n, lines, K, kind, causal):
    """every call of one case, once: the results on the host, shared by the tests below and never written"""
    import torch
    x, sections, g = cases.case(hop, n, lines, K, kind, causal)
    stride = cases.STRIDES.get((lines, n))
    count = loops.frames_count(n, hop)
    fresh = lambda: nan_lines(lines, n, stride)      # noqa: E731
    r = {}
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        dx, dg, ds = device_lines(x, stride), device_lines(g, stride), device_sections(sections)
        y = plan.execute_cascade_frames(dx, ds, hop, fresh())
        y_keep, kept = plan.execute_cascade_frames(dx, ds, hop, fresh(), keep=True, kept=[fresh() for _ in range(K - 1)])
        signals = [tuple(rfa.expand_frames(f, hop, n, out=plan._like(dx)) for f in s) for s in ds]
        y_signals = plan.execute_cascade(dx, signals)
        y_signals_keep, kept_signals = plan.execute_cascade_keep(dx, signals)
        only_x, none = plan.backward_cascade_frames(None, ds, hop, None, None, dg, fresh())
        assert none is None
        gin, grads = plan.backward_cascade_frames(dx, ds, hop, kept, y_keep, dg, fresh(), nan_grads(lines, count, K))
        gin2, grads2 = plan.backward_cascade_frames(dx, ds, hop, kept, y_keep, dg, fresh(), nan_grads(lines, count, K))
        only_x_signals, _ = plan.backward_cascade_kept(None, signals, None, None, dg)
        gin_signals, per_sample = plan.backward_cascade_kept(dx, signals, kept_signals, y_signals_keep, dg, None,
                                                            [tuple(plan._like(dx) for _ in range(5)) for _ in range(K)])
        torch.cuda.synchronize()
        for name, t in (("out", y), ("out keep", y_keep), ("out signals", y_signals), ("out signals keep", y_signals_keep), ("only_x", only_x),
                        ("grad_x", gin), ("grad_x again", gin2), ("only_x signals", only_x_signals), ("grad_x signals", gin_signals)):
            r[name] = host(t, lines)
        for k in range(K - 1):
            r[f"kept {k}"], r[f"kept {k} signals"] = host(kept[k], lines), host(kept_signals[k], lines)
        flat = lambda per_section: [t for s in per_section for t in s]      # noqa: E731
        for name, a, b, p in zip(cases.names(K)[2:], flat(grads), flat(grads2), flat(per_sample)):
            r[name], r[name + " again"], r[name + " per sample"] = host(a, lines), host(b, lines), host(p, lines)
        if lines > 1:      # what lies between the lines and behind the frames
            r["between the lines"] = all(bool(torch.isnan(t._base[:, n:]).all()) for t in (y, y_keep, gin, *kept))
            r["behind the frames"] = all(bool(torch.isnan(t._base[:, count:]).all()) for t in flat(grads))
    return r


# ---- 1: the cascade on the expanded signals -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,n,lines,K,kind,causal", cases.ALL)
def test_forward_is_the_cascade_on_the_expanded_signals_bit_for_bit(hop, n, lines, K, kind, causal):
    r = run(hop, n, lines, K, kind, causal)
    assert not np.isnan(r["out"]).any()
    np.testing.assert_array_equal(bits(r["out"]), bits(r["out signals"]))
    np.testing.assert_array_equal(bits(r["out keep"]), bits(r["out"]))      # keeping or not
    np.testing.assert_array_equal(bits(r["out signals keep"]), bits(r["out"]))
    for k in range(K - 1):
        assert not np.isnan(r[f"kept {k}"]).any()
        np.testing.assert_array_equal(bits(r[f"kept {k}"]), bits(r[f"kept {k} signals"]), f"kept {k}")


# ---- 2: one section -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_one_section_is_the_section_on_frames(kind, causal):
    """K = 1: out, grad_in and the frame gradients are execute_biquad_frames' / backward_biquad_frames', and so are the launches"""
    import torch
    hop, n = 64, 4100
    x, sections, g = cases.case(hop, n, 1, 1, kind, causal)
    r = run(hop, n, 1, 1, kind, causal)
    count = loops.frames_count(n, hop)
    with rfa.Var2Plan(n, causal=causal) as plan:
        dx, dg, ds = device_lines(x), device_lines(g), device_sections(sections)
        y, times = plan.execute_biquad_frames_timed(dx, ds[0], hop)
        only_x, _ = plan.backward_biquad_frames(dx, ds[0], hop, None, dg)
        gin, grads, backward_times = plan.backward_biquad_frames_timed(dx, ds[0], hop, y, dg, None, nan_grads(1, count, 1)[0])
        _, cascade_times = plan.execute_cascade_frames_timed(dx, ds, hop)
        *_, cascade_only_x_times = plan.backward_cascade_frames_timed(dx, ds, hop, None, None, dg)
        *_, cascade_backward_times = plan.backward_cascade_frames_timed(dx, ds, hop, None, y, dg, None, nan_grads(1, count, 1))
        torch.cuda.synchronize()
    assert [name for name, _ in cascade_times] == [name for name, _ in times] and len(times) == 3
    assert [name for name, _ in cascade_backward_times] == [name for name, _ in backward_times] and len(backward_times) == 5
    assert [name for name, _ in cascade_only_x_times] == [name for name, _ in backward_times[:4]]
    np.testing.assert_array_equal(bits(r["out"]), bits(host(y, 1)))
    np.testing.assert_array_equal(bits(r["only_x"]), bits(host(only_x, 1)))
    np.testing.assert_array_equal(bits(r["grad_x"]), bits(host(gin, 1)))
    for name, t in zip(cases.names(1)[2:], grads):
        np.testing.assert_array_equal(bits(r[name]), bits(host(t, 1)), name)


# ---- 3: no feedback -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("hop,n,lines,K", [(64, 68, 1, 2), (64, 4100, 1, 3), (4096, 8196, 1, 4), (64, 4100, 3, 2)])
def test_zero_feedback_is_chained_sections_on_frames(hop, n, lines, K, causal):
    """all a1, a2 frames 0: the state that enters a tile IS the neighbouring tile's samples, and the result is K chained
    execute_biquad_frames calls bit for bit -- the link's neighbour indexing at tile, group and interval edges"""
    import torch
    x, sections, _ = cases.case(hop, n, lines, K, "resonator", causal)
    stride = cases.STRIDES.get((lines, n))
    zero = np.zeros_like(sections[0][0])
    sections = [(b0, b1, b2, zero, zero) for b0, b1, b2, _, _ in sections]
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        dx, ds = device_lines(x, stride), device_sections(sections)
        got, kept = plan.execute_cascade_frames(dx, ds, hop, keep=True)
        want = dx
        for k in range(K):
            want = plan.execute_biquad_frames(want, ds[k], hop)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(bits(host(got if k == K - 1 else kept[k], lines)), bits(host(want, lines)), f"section {k}")


# ---- 4: grad_in -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,n,lines,K,kind,causal", cases.ALL)
def test_grad_in_is_the_kept_backwards_on_the_expanded_signals_bit_for_bit(hop, n, lines, K, kind, causal):
    r = run(hop, n, lines, K, kind, causal)
    assert not np.isnan(r["grad_x"]).any()
    np.testing.assert_array_equal(bits(r["grad_x"]), bits(r["grad_x signals"]))
    np.testing.assert_array_equal(bits(r["only_x"]), bits(r["only_x signals"]))      # in, out and kept were None
    np.testing.assert_array_equal(bits(r["only_x"]), bits(r["grad_x"]))              # with or without the frame gradients


# ---- 5: the contraction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,n,lines,K,kind,causal", cases.ALL)
def test_frame_gradients_are_the_f64_contraction_rounded_once(hop, n, lines, K, kind, causal):
    """g32: the per-sample gradients rf_var2_plan_backward_cascade_kept stores on the expanded signals; s = contract(g32) in f64.
    |got - s| <= 2 (2^-24 |s| + 2^-36 sum |w g32|): one rounding to f32, and f64 sums of at most 2^17 exact products"""
    r = run(hop, n, lines, K, kind, causal)
    count = loops.frames_count(n, hop)
    worst = 0.0
    for name in cases.names(K)[2:]:
        g32 = r[name + " per sample"]
        s = loops.contract(g32, hop, count, np.float64)
        bound = 2 * (2.0 ** -24 * np.abs(s) + 2.0 ** -36 * loops.contraction_bound(g32, hop, count))
        err = np.abs(r[name].astype(np.float64) - s)
        share = float(np.max(err / np.maximum(bound, 1e-300)))
        worst = max(worst, share)
        assert r[name].shape == (lines, count) and not np.isnan(r[name]).any()
        assert np.all(err <= bound), f"{name}: |got - s| up to {share:.2f} x the bound"
    SHARES[hop, n, lines, K, kind, causal] = worst
    print(f"hop {hop} {n} x {lines} K={K} {kind} {name_of(causal)}: worst |got - s| / bound {worst:.3f}")
    write_profile("cascade_frames_contraction.txt", [f"{key}: worst |got - s| / bound {v:.3f}\n" for key, v in SHARES.items()]
                  + [f"worst of {len(SHARES)} of {len(cases.ALL)} cases: {max(SHARES.values()):.3f}\n"])


# ---- 6: end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,n,lines,K,kind,causal", cases.UNDER_THE_BAR)
def test_against_f64_loops(hop, n, lines, K, kind, causal):
    r = run(hop, n, lines, K, kind, causal)
    want = cases.expected(hop, n, lines, K, kind, causal)
    worst = 0.0
    for name in cases.names(K):
        cases.assert_under_bar(r[name], want[name], f"hop {hop} {n} x {lines} K={K} {kind} {name_of(causal)} {name}")
        reference, err32, peak = want[name]
        worst = max(worst, cases._figure(r[name], reference, peak) / max(4 * err32, 1e-6))
    RATIOS[hop, n, lines, K, kind, causal] = worst
    write_profile("cascade_frames_ratios.txt", [f"{key}: worst err / bar {v:.3f}\n" for key, v in RATIOS.items()]
                  + [f"worst of {len(RATIOS)} of {len(cases.UNDER_THE_BAR)} cases: {max(RATIOS.values()):.3f} of the bar, max(4 x the f32 serial loops', 1e-6)\n"])


# ---- 7: reproducibility, calls of every kind on one plan ------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,n,lines,K,kind,causal", cases.ALL)
def test_two_backward_calls_give_the_same_bits(hop, n, lines, K, kind, causal):
    r = run(hop, n, lines, K, kind, causal)
    for name in cases.names(K)[1:]:
        np.testing.assert_array_equal(bits(r[name]), bits(r[name + " again"]))


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_backward_calls_of_every_kind_mix_on_one_plan(causal):
    """backward_cascade_kept, backward_biquad_frames at hop 4096, backward_cascade_frames at K = 2 and at K = 4 (hop 64) on one
    plan in that order and reversed -- the slab regrows in both orders -- every call's results the bits it gives alone"""
    import torch
    n = 4100
    x, sections, g = cases.case(64, n, 1, 3, "resonator", causal)
    _, extra, _ = cases.case(64, n, 1, 2, "near one", causal)
    four = sections + extra[:1]
    big = cases.frames_of("resonator", 1, loops.frames_count(n, 4096), 4096, np.random.default_rng(5))
    dx, dg = device_lines(x), device_lines(g)

    def frame_grads(frames_of_sections):
        return [tuple(torch.full_like(f, float("nan")) for f in s) for s in frames_of_sections]

    def kept_signals(plan):
        signals = [tuple(rfa.expand_frames(f, 64, n) for f in s) for s in device_sections(sections[:2])]
        y, kept = plan.execute_cascade_keep(dx, signals)
        gin, grads = plan.backward_cascade_kept(dx, signals, kept, y, dg, None, [tuple(plan._like(dx) for _ in range(5)) for _ in range(2)])
        return [gin] + [t for s in grads for t in s]

    def one_section(plan):
        df = tuple(device_frames(f) for f in big)
        y = plan.execute_biquad_frames(dx, df, 4096)
        gin, grads = plan.backward_biquad_frames(dx, df, 4096, y, dg, None, frame_grads([df])[0])
        return [gin, *grads]

    def cascade(plan, which):
        ds = device_sections(which)
        y, kept = plan.execute_cascade_frames(dx, ds, 64, keep=True)
        gin, grads = plan.backward_cascade_frames(dx, ds, 64, kept, y, dg, None, frame_grads(ds))
        return [gin] + [t for s in grads for t in s]
    calls = [kept_signals, one_section, lambda plan: cascade(plan, sections[:2]), lambda plan: cascade(plan, four)]
    alone = []
    for call in calls:
        with rfa.Var2Plan(n, causal=causal) as plan:
            alone.append([host(t, 1) for t in call(plan)])
            torch.cuda.synchronize()
    for order in (range(4), reversed(range(4))):
        with rfa.Var2Plan(n, causal=causal) as plan:
            for i in order:
                got = [host(t, 1) for t in calls[i](plan)]
                assert len(got) == len(alone[i])
                for j, (a, b) in enumerate(zip(got, alone[i])):
                    assert not np.isnan(a).any()
                    np.testing.assert_array_equal(bits(a), bits(b), f"call {i}, result {j}")
            assert plan.backward_cascade_frames_bytes(4, 64) == 2 * 4 * n + 4 * 80 * 65


# ---- 8: guards ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("hop,n,lines,K", [(64, 4100, 3, 2), (64, 196, 70, 2)])
def test_nothing_is_written_between_the_lines_or_behind_the_frames(hop, n, lines, K, causal):
    """strided lines, frame rows F + 3 apart: out, the kept signals, grad_in and the frame gradients began as NaN, are fully
    written, and the NaN between the lines and in the frame padding is untouched"""
    r = run(hop, n, lines, K, "resonator", causal)
    assert r["between the lines"] and r["behind the frames"]
    for name in cases.names(K):
        assert not np.isnan(r[name]).any(), name


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_the_backward_changes_nothing_it_reads(causal):
    import torch
    hop, n, K = 64, 4100, 3
    x, sections, g = cases.case(hop, n, 1, K, "resonator", causal)
    count = loops.frames_count(n, hop)
    with rfa.Var2Plan(n, causal=causal) as plan:
        dx, dg, ds = device_lines(x), device_lines(g), device_sections(sections)
        y, kept = plan.execute_cascade_frames(dx, ds, hop, keep=True)
        torch.cuda.synchronize()
        before = [t.clone() for t in (dx, dg, y, *kept, *(f for s in ds for f in s))]
        plan.backward_cascade_frames(dx, ds, hop, kept, y, dg, None, nan_grads(1, count, K))
        torch.cuda.synchronize()
        for a, b in zip(before, (dx, dg, y, *kept, *(f for s in ds for f in s))):
            np.testing.assert_array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))


@pytest.mark.parametrize("causal", DIRECTIONS)
def test_a_nan_in_one_line_reaches_no_other_line(causal):
    import torch
    hop, n, lines, K = 64, 4100, 3, 2
    stride = cases.STRIDES[lines, n]
    x, sections, g = cases.case(hop, n, lines, K, "resonator", causal)
    r = run(hop, n, lines, K, "resonator", causal)
    count = loops.frames_count(n, hop)
    poisoned = np.array(x)
    poisoned[1, n // 2] = np.nan
    with rfa.Var2Plan(n, lines=lines, causal=causal, stride=stride) as plan:
        dx, dg, ds = device_lines(poisoned, stride), device_lines(g, stride), device_sections(sections)
        y, kept = plan.execute_cascade_frames(dx, ds, hop, keep=True)
        gin, grads = plan.backward_cascade_frames(dx, ds, hop, kept, y, dg, None, nan_grads(lines, count, K))
        torch.cuda.synchronize()
    got = dict(zip(cases.names(K), [host(t, lines) for t in (y, gin, *(t for s in grads for t in s))]))
    assert np.isnan(got["out"][1]).any() and np.isnan(got["grad_b0_0"][1]).any() and np.isnan(got["grad_a1_1"][1]).any()
    for name in cases.names(K):
        for line in (0, 2):
            np.testing.assert_array_equal(bits(got[name][line]), bits(r[name][line]), err_msg=f"{name} line {line}")


# ---- 9: autograd ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", DIRECTIONS)
@pytest.mark.parametrize("lines", [1, 2])
def test_biquad_cascade_frames_against_chained_biquad_scan_frames(lines, causal):
    """N = 101 (padded to 104), hop 64, K = 2: biquad_cascade_frames under autograd and K chained biquad_scan_frames under
    autograd, both under the bar against the f64 loops; with x alone requiring a gradient nothing but the frames is saved"""
    import torch
    n, hop, K = 101, 64, 2
    count = loops.frames_count(n, hop)
    rng = np.random.default_rng(101 + lines)
    x, g = ((rng.random((lines, n)) * 2 - 1).astype(np.float32) for _ in range(2))
    sections = [cases.frames_of("resonator", lines, count, hop, rng) for _ in range(K)]
    want = cases.reference([(x, sections, g)], hop, [causal])[0]
    squeeze = (lambda a: a[0]) if lines == 1 else (lambda a: a)
    dg = torch.from_numpy(squeeze(g)).cuda()

    def leaves():
        return (torch.from_numpy(squeeze(x)).cuda().requires_grad_(),
                [tuple(torch.from_numpy(squeeze(f)).cuda().requires_grad_() for f in s) for s in sections])
    dx, ds = leaves()
    out = rfa.biquad_cascade_frames(dx, ds, hop, causal=causal)
    assert tuple(out.shape) == tuple(dx.shape)
    out.backward(dg)
    ex, es = leaves()
    chained = ex
    for s in es:
        chained = rfa.biquad_scan_frames(chained, *s, hop, causal=causal)
    chained.backward(dg)
    torch.cuda.synchronize()
    new = [out.detach(), dx.grad] + [f.grad for s in ds for f in s]
    old = [chained.detach(), ex.grad] + [f.grad for s in es for f in s]
    for a, b, name in zip(new, old, cases.names(K)):
        cases.assert_under_bar(host(a, lines), want[name], f"biquad_cascade_frames {lines} x {n} {name_of(causal)} {name}")
        cases.assert_under_bar(host(b, lines), want[name], f"chained biquad_scan_frames {lines} x {n} {name_of(causal)} {name}")
    # the input's gradient alone: the same bits, and the frames are all that is saved
    saved = []
    x2 = torch.from_numpy(squeeze(x)).cuda().requires_grad_()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(tuple(t.shape)) or t, lambda t: t):
        out2 = rfa.biquad_cascade_frames(x2, [tuple(f.detach() for f in s) for s in ds], hop, causal=causal)
    out2.backward(dg)
    frame_shape = (count,) if lines == 1 else (lines, count)
    assert saved == [frame_shape] * (5 * K), saved
    np.testing.assert_array_equal(bits(out2.detach().cpu().numpy()), bits(out.detach().cpu().numpy()))
    np.testing.assert_array_equal(bits(x2.grad.cpu().numpy()), bits(dx.grad.cpu().numpy()))


# ---- 10: launches and refusals ----------------------------------------------------------------------------------------------------------
def test_launch_names_counts_and_call_refusals():
    import torch
    n, hop = 4100, 64
    count = rfa.frames_count(n, hop)
    x = torch.zeros(n, device="cuda")
    new = lambda: torch.empty_like(x)      # noqa: E731
    section = tuple(torch.full((count,), v, device="cuda") for v in (1.0, -0.5, 0.25, -0.5, 0.25))
    five = lambda K: [tuple(torch.empty(count, device="cuda") for _ in range(5)) for _ in range(K)]      # noqa: E731
    with rfa.Var2Plan(n) as plan:
        for K in (2, 3, 16):
            sections = [section] * K
            for keep, link in ((False, "var2_frames_link_1d"), (True, "var2_frames_link_keep_1d")):
                *_, times = plan.execute_cascade_frames_timed(x, sections, hop, keep=keep)
                want = ["var2_biquad_frames_tails_1d"] + ["var2_carry_1d", link] * (K - 1) + ["var2_carry_1d", "var2_frames_pass2_1d"]
                assert [name for name, _ in times] == want and len(want) == 2 * K + 1 == plan.cascade_frames_num_kernels(K)
                assert all(ms >= 0 for _, ms in times)
            y, kept = plan.execute_cascade_frames(x, sections, hop, keep=True)
            last = ["var2_carry_1d", "var2_adj_frames_pass2_1d", "var2_biquad_frames_grad_1d"]
            want = ["var2_adj_frames_tails_1d"] + ["var2_carry_1d", "var2_adj_frames_link_1d"] * (K - 1) + last
            *_, times = plan.backward_cascade_frames_timed(None, sections, hop, None, None, x)
            assert [name for name, _ in times] == want and len(want) == 2 * K + 2 == plan.backward_cascade_frames_num_kernels(K, False)
            want = (["var2_adj_frames_tails_1d"] + ["var2_carry_1d", "var2_adj_frames_link_keep_1d", "var2_frames_coef_1d"] * (K - 1) + last
                    + ["var2_frames_fold_cascade_1d"])
            *_, times = plan.backward_cascade_frames_timed(x, sections, hop, kept, y, x, None, five(K))
            assert [name for name, _ in times] == want and len(want) == 3 * K + 2 == plan.backward_cascade_frames_num_kernels(K, True)
        assert plan.backward_cascade_frames_bytes(2, hop) == 2 * 4 * n + 2 * 80 * 65
        g = torch.ones(n, device="cuda")
        two = [section, section]
        y, kept = plan.execute_cascade_frames(x, two, hop, keep=True)
        gin, _ = plan.backward_cascade_frames(x, two, hop, kept, y, g, g, five(2))      # grad_in == grad_out
        assert gin.data_ptr() == g.data_ptr()
        mixed = five(2)
        mixed[1] = (mixed[1][0], mixed[1][1], None, mixed[1][3], mixed[1][4])
        refused = [
            lambda: plan.execute_cascade_frames(x, two, hop, x),                                       # in == out
            lambda: plan.execute_cascade_frames(x, two, hop, None, kept=[x]),                          # a kept signal that is the input
            lambda: plan.execute_cascade_frames(x, two, hop, y, kept=[y]),                             # a kept signal that is the output
            lambda: plan.execute_cascade_frames(x, [], hop),                                           # no section
            lambda: plan.backward_cascade_frames(x, two, hop, None, y, g, None, five(2)),              # frame gradients need the kept signals
            lambda: plan.backward_cascade_frames(x, two, hop, kept, None, g, None, five(2)),           # and out
            lambda: plan.backward_cascade_frames(None, two, hop, kept, y, g, None, five(2)),           # and in
            lambda: plan.backward_cascade_frames(x, two, hop, kept, y, g, kept[0], five(2)),           # a gradient written over a kept signal
            lambda: plan.backward_cascade_frames(x, two, hop, kept, y, g, None, [section, five(1)[0]]),      # frame gradients over the frames
        ]
        for i, call in enumerate(refused):
            with pytest.raises(rfa.RecFilterError) as e:
                call()
            assert e.value.status == rfa.capi.RF_ERR_INVALID_ARG, i
            assert len(str(e.value)) > 15, i
        for call in (lambda: plan.execute_cascade_frames(x, two, 480), lambda: plan.execute_cascade_frames(x, [section[:4]], hop),
                     lambda: plan.execute_cascade_frames(x, [tuple(f[:-1] for f in section)] * 2, hop),
                     lambda: plan.backward_cascade_frames(x, two, hop, kept, y, g, None, mixed)):
            with pytest.raises((ValueError, TypeError, AttributeError)):
                call()
        torch.cuda.synchronize()


# ---- 11: the C++ front-end --------------------------------------------------------------------------------------------------------------
def test_cpp_frontend_cascade_frames(tmp_path):
    """RecFilterVarying2::realize_cascade_frames / gradient_cascade_frames on a signal of 12356 samples at hops 64 and 8192, three
    sections, both directions, against the C calls bit for bit; compiled here with the command line of tests/cpp/Makefile"""
    src = os.path.join(ROOT, "tests", "cpp", "test_frontend_cascade_frames.cpp")
    exe = str(tmp_path / "test_frontend_cascade_frames")
    lib = os.path.join(ROOT, "recfilter_amd")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", src, "-o", exe, "-L" + lib, "-lrecfilter_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "cascade-frames-frontend-ok" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
