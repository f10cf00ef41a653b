#!/usr/bin/env python3
"""The cascade on frames with a state that enters and leaves the call (rf_var2_plan_execute_cascade_frames_stream,
kernels_var2_signal.hip) beside the call without one, everything alternating in ONE process (the protocol of var2_probe.py: medians
of `rounds` rounds of `steps` steps, with the rounds' min and max).

    python tools/probes/var2_stream_probe.py [--cases N:LINES ...] [--hops 64 512 4096] [--sections 2 4 8] [--steps 10] [--rounds 5]
                                             [--long 268435456] [--long-sections 8] [--chunks 1048576 4194304 16777216] [--out FILE]

Per case (default: 10^7, 2^24 and 2^28 samples on one line, 4096 lines of 4096 samples), hop and K, a causal plan:
  (a) the spread of execute_cascade_frames from round to round, then execute_cascade_frames_stream (a state enters, a state
      leaves) on the same plan: a stream call whose median is above the existing call's median plus that spread is REPORTED with
      its kernels beside their twins (execute_cascade_frames_stream_timed against execute_cascade_frames_timed);
  (b) the same with keeping;
  (c) backward_cascade_frames_stream against backward_cascade_frames, without and with frame gradients (`probe_backward`).
Then one long signal (--long samples, --long-sections sections, hop 64) filtered in chunks of --chunks samples through one plan
per chunk length and two state buffers that swap roles, against one call on the whole signal: the time of the forward and the peak
of torch's device memory above the input, the frames and the output (a chunked call writes into its slice of the output); then a
training step on it, whole against chunk by chunk with the state detached between the chunks (`training`)."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

med = statistics.median
out_file = None


def say(line=""):
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n")
        out_file.flush()


def spread(v):
    return f"(min {min(v):.4f}, max {max(v):.4f})"


def timed(fn, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def inputs(n, lines, hop, K, seed=35):
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(seed)
    count = rfa.frames_count(n, hop)
    shape, fshape = ((n,), (count,)) if lines == 1 else ((lines, n), (lines, count))
    rand = lambda s: torch.rand(s, device="cuda", generator=gen)      # noqa: E731

    def section():
        theta, r = 0.2 + (math.pi - 0.4) * rand(fshape), 0.5 + 0.48 * rand(fshape)
        phi, q, k = 0.2 + (math.pi - 0.4) * rand(fshape), 0.3 + 0.7 * rand(fshape), 0.5 + 0.5 * rand(fshape)
        return tuple(t.contiguous() for t in (k, -2 * k * q * torch.cos(phi), k * q * q, -2 * r * torch.cos(theta), r * r))
    return rand(shape) * 2 - 1, [section() for _ in range(K)]


def per_kernel(times):
    """{name: the summed ms of its launches}"""
    out = {}
    for name, ms in times:
        out[name] = out.get(name, 0.0) + ms
    return out


def probe(n, lines, hop, K, steps, rounds):
    import torch
    import recfilter_amd as rfa
    x, sections = inputs(n, lines, hop, K)
    state_shape = (K + 1, 2) if lines == 1 else (lines, K + 1, 2)
    say(f"== {n} samples x {lines} line(s), hop {hop}, K = {K}")
    with rfa.Var2Plan(n, lines=lines, causal=True) as plan:
        out = torch.empty_like(x)
        kept = [torch.empty_like(x) for _ in range(K - 1)]
        entering = torch.rand(state_shape, device="cuda") * 0.1
        leaving = torch.empty_like(entering)
        routes = {
            "plain": lambda: plan.execute_cascade_frames(x, sections, hop, out),
            "stream": lambda: plan.execute_cascade_frames_stream(x, sections, hop, entering, out, state_out=leaving),
            "plain keep": lambda: plan.execute_cascade_frames(x, sections, hop, out, kept=kept),
            "stream keep": lambda: plan.execute_cascade_frames_stream(x, sections, hop, entering, out, kept=kept, state_out=leaving),
        }
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in routes}
        for _ in range(rounds):
            for name, fn in routes.items():
                ms[name].append(timed(fn, steps))
        kernels = {"plain": [], "stream": [], "plain keep": [], "stream keep": []}
        for _ in range(rounds):
            kernels["plain"].append(per_kernel(plan.execute_cascade_frames_timed(x, sections, hop, out)[-1]))
            kernels["stream"].append(per_kernel(plan.execute_cascade_frames_stream_timed(x, sections, hop, entering, out, state_out=leaving)[-1]))
            kernels["plain keep"].append(per_kernel(plan.execute_cascade_frames_timed(x, sections, hop, out, kept=kept)[-1]))
            kernels["stream keep"].append(per_kernel(plan.execute_cascade_frames_stream_timed(x, sections, hop, entering, out, kept=kept, state_out=leaving)[-1]))
    for plain, stream in (("plain", "stream"), ("plain keep", "stream keep")):
        own = max(ms[plain]) - min(ms[plain])
        ratio = med(ms[stream]) / med(ms[plain])
        above = med(ms[stream]) > med(ms[plain]) + own
        say(f"     {plain:11s} {med(ms[plain]):9.4f} ms {spread(ms[plain])}, spread {own:.4f};  {stream:11s} {med(ms[stream]):9.4f} ms {spread(ms[stream])}"
            f"   stream / plain {ratio:.3f}{'   ABOVE the median plus the spread' if above else ''}")
        if above:
            for name in kernels[stream][0]:
                twin = name.replace("_stream_1d", "_1d")
                a, b = [r[name] for r in kernels[stream]], [r[twin] for r in kernels[plain]]
                say(f"         {name:40s} {med(a):9.4f} ms {spread(a)}   {twin:34s} {med(b):9.4f} ms {spread(b)}   {med(a) / med(b):.3f}")
    return med(ms["stream"]) / med(ms["plain"])


def probe_backward(n, lines, hop, K, steps, rounds):
    """backward_cascade_frames_stream (a state entered, a gradient of the leaving state is added, grad_state_in is formed) against
    backward_cascade_frames on the same plan and the same kept signals, without and with frame gradients; rows as in `probe`"""
    import torch
    import recfilter_amd as rfa
    x, sections = inputs(n, lines, hop, K)
    g = torch.rand_like(x) * 2 - 1
    state_shape = (K + 1, 2) if lines == 1 else (lines, K + 1, 2)
    with rfa.Var2Plan(n, lines=lines, causal=True) as plan:
        entering = torch.rand(state_shape, device="cuda") * 0.1
        gso, gsi = torch.rand(state_shape, device="cuda") * 0.1, torch.empty(state_shape, device="cuda")
        out, kept, _ = plan.execute_cascade_frames_stream(x, sections, hop, entering, keep=True)
        gin = torch.empty_like(x)
        grads = [tuple(torch.empty_like(f) for f in s) for s in sections]
        calls = {
            "backward": (plan.backward_cascade_frames, plan.backward_cascade_frames_timed, (None, sections, hop, None, None, g, gin), ()),
            "stream backward": (plan.backward_cascade_frames_stream, plan.backward_cascade_frames_stream_timed, (None, sections, hop, None, None, g, gin),
                                (None, None, gso, gsi)),
            "backward+grads": (plan.backward_cascade_frames, plan.backward_cascade_frames_timed, (x, sections, hop, kept, out, g, gin, grads), ()),
            "stream backward+grads": (plan.backward_cascade_frames_stream, plan.backward_cascade_frames_stream_timed,
                                      (x, sections, hop, kept, out, g, gin, grads), (entering, gso, gsi)),
        }
        for call, _, args, more in calls.values():
            call(*args, *more)
        torch.cuda.synchronize()
        ms = {name: [] for name in calls}
        for _ in range(rounds):
            for name, (call, _, args, more) in calls.items():
                ms[name].append(timed(lambda: call(*args, *more), steps))
        kernels = {name: [per_kernel(call_timed(*args, *more)[-1]) for _ in range(rounds)] for name, (_, call_timed, args, more) in calls.items()}
    worst = 0.0
    for plain, stream in (("backward", "stream backward"), ("backward+grads", "stream backward+grads")):
        own = max(ms[plain]) - min(ms[plain])
        ratio = med(ms[stream]) / med(ms[plain])
        worst = max(worst, ratio)
        above = med(ms[stream]) > med(ms[plain]) + own
        say(f"     {plain:14s} {med(ms[plain]):9.4f} ms {spread(ms[plain])}, spread {own:.4f};  {stream:21s} {med(ms[stream]):9.4f} ms {spread(ms[stream])}"
            f"   stream / plain {ratio:.3f}{'   ABOVE the median plus the spread' if above else ''}")
        if above:
            for name in kernels[stream][0]:
                twin = name.replace("_stream_1d", "_1d")
                a, b = [r[name] for r in kernels[stream]], [r[twin] for r in kernels[plain]]
                say(f"         {name:40s} {med(a):9.4f} ms {spread(a)}   {twin:34s} {med(b):9.4f} ms {spread(b)}   {med(a) / med(b):.3f}")
    return worst


def chunked(n, K, hop, chunks, rounds):
    """one long signal in chunks against one call: the forward's time and its peak memory above the signal, the frames and the output"""
    import torch
    import recfilter_amd as rfa
    x, sections = inputs(n, 1, hop, K)
    out = torch.empty_like(x)
    say(f"== {n} samples x 1 line, hop {hop}, K = {K}, in chunks")

    def measure(fn):
        fn()
        torch.cuda.synchronize()
        ms = [timed(fn, 1) for _ in range(rounds)]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return ms, torch.cuda.max_memory_allocated() - before
    with rfa.Var2Plan(n, causal=True) as plan:
        whole_ms, whole_peak = measure(lambda: plan.execute_cascade_frames(x, sections, hop, out))
        whole_plan = plan.workspace_bytes
        reference = out.clone()
    say(f"     one call                   {med(whole_ms):9.4f} ms {spread(whole_ms)}   torch peak above the arrays {whole_peak / 2**20:8.2f} MiB, "
        f"the plan's workspace {whole_plan / 2**20:8.2f} MiB")
    for m in chunks:
        if n % m or m % hop:
            say(f"     chunks of {m}: not a divisor of {n} on the frame grid, skipped")
            continue
        count = rfa.frames_count(m, hop)
        with rfa.Var2Plan(m, causal=True) as plan:
            states = [torch.empty((K + 1, 2), device="cuda") for _ in range(2)]

            def run():
                entering = None
                for i, start in enumerate(range(0, n, m)):
                    own = [tuple(f[start // hop:start // hop + count] for f in s) for s in sections]
                    plan.execute_cascade_frames_stream(x[start:start + m], own, hop, entering, out[start:start + m], state_out=states[i % 2])
                    entering = states[i % 2]
            ms, peak = measure(run)
            err = float((out - reference).abs().max() / reference.abs().max())
            say(f"     chunks of {m:10d} ({n // m:4d}) {med(ms):9.4f} ms {spread(ms)}   torch peak above the arrays {peak / 2**20:8.2f} MiB, "
                f"the plan's workspace {plan.workspace_bytes / 2**20:8.2f} MiB   chunked / one call {med(ms) / med(whole_ms):.3f}   "
                f"max |chunked - one call| / peak {err:.2e}")


def training(n, K, hop, chunks, rounds):
    """a training step on one long signal -- x and all 5 K frame tensors require gradients, the loss is the sum of the result --
    through biquad_cascade_frames on the whole signal against biquad_cascade_frames_stream chunk by chunk with the state detached
    between the chunks (truncated back-propagation: forward and backward of one chunk before the next): time, and the peak of
    torch's device memory above x, the frames and their gradients"""
    import torch
    import recfilter_amd as rfa
    x, sections = inputs(n, 1, hop, K)
    x.requires_grad_(True)
    sections = [tuple(f.requires_grad_(True) for f in s) for s in sections]
    leaves = [x] + [f for s in sections for f in s]
    say(f"== a training step, {n} samples x 1 line, hop {hop}, K = {K}")

    def whole():
        rfa.biquad_cascade_frames(x, sections, hop).sum().backward()

    def chunked_step(m):
        # every chunk's x and frames are leaves of their own, made beforehand: the gradient of a slice of one big leaf is a tensor
        # of the big leaf's size per chunk, which would measure torch and not the library
        count = rfa.frames_count(m, hop)
        with torch.no_grad():
            parts = [(x[start:start + m].clone().requires_grad_(True),
                      [tuple(f[start // hop:start // hop + count].clone().requires_grad_(True) for f in s) for s in sections]) for start in range(0, n, m)]

        def run():
            state = None
            for own_x, own in parts:
                y, state = rfa.biquad_cascade_frames_stream(own_x, own, hop, state)
                y.sum().backward()
                state = state.detach()
        return run

    def measure(fn):
        fn()      # (the gradients exist from here on: they are not part of the peak)
        torch.cuda.synchronize()
        ms = [timed(fn, 1) for _ in range(rounds)]
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return ms, torch.cuda.max_memory_allocated() - before
    whole_ms, whole_peak = measure(whole)
    say(f"     one call                   {med(whole_ms):9.4f} ms {spread(whole_ms)}   torch peak above the leaves {whole_peak / 2**20:9.2f} MiB")
    for m in chunks:
        if n % m or m % hop:
            continue
        for t in leaves:
            t.grad = None
        step = chunked_step(m)
        ms, peak = measure(step)
        del step
        say(f"     chunks of {m:10d} ({n // m:4d}) {med(ms):9.4f} ms {spread(ms)}   torch peak above the leaves {peak / 2**20:9.2f} MiB"
            f"   chunked / one call {med(ms) / med(whole_ms):.3f} in time, {peak / max(whole_peak, 1):.3f} in memory")


def main():
    global out_file
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["10000000:1", "16777216:1", "268435456:1", "4096:4096"])
    ap.add_argument("--hops", nargs="+", type=int, default=[64, 512, 4096])
    ap.add_argument("--sections", nargs="+", type=int, default=[2, 4, 8])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--long", type=int, default=1 << 28)
    ap.add_argument("--long-sections", type=int, default=8)
    ap.add_argument("--chunks", nargs="+", type=int, default=[1 << 20, 1 << 22, 1 << 24])
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.out:
        out_file = open(a.out, "w")
    say(f"var2_stream_probe: {torch.cuda.get_device_name(0)}; steps {a.steps}, rounds {a.rounds}; medians over the rounds (min, max)")
    ratios, backward = [], []
    for case in a.cases:
        n, lines = (int(v) for v in case.split(":"))
        for hop in a.hops:
            for K in a.sections:
                ratios.append(probe(n, lines, hop, K, a.steps, a.rounds))
                torch.cuda.empty_cache()
                backward.append(probe_backward(n, lines, hop, K, a.steps, a.rounds))
                torch.cuda.empty_cache()
    if ratios:
        say(f"stream / plain over {len(ratios)} shapes: {min(ratios):.3f} .. {max(ratios):.3f}, median {med(ratios):.3f}")
        say(f"stream backward / backward, the larger of without and with frame gradients: {min(backward):.3f} .. {max(backward):.3f}, median {med(backward):.3f}")
    if a.long:
        chunked(a.long, a.long_sections, 64, a.chunks, a.rounds)
        torch.cuda.empty_cache()
        training(a.long, a.long_sections, 64, a.chunks, a.rounds)


if __name__ == "__main__":
    main()
