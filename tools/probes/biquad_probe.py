#!/usr/bin/env python3
"""The time-varying direct-form-I section on signals (rf_var2_plan_execute_biquad / _backward_biquad, kernels_var2_signal.hip):
whole-step and per-kernel times beside the measured copy rate, the all-pole step and the only route there was before, everything
alternating in ONE process (the protocol of var2_probe.py: medians of `rounds` rounds of `steps` steps, with the rounds' min and max).

    python tools/probes/biquad_probe.py [--cases N:LINES ...] [--steps 10] [--rounds 5] [--out FILE]

Per case (default: 10^7, 2^24 and 2^28 samples on one line, 4096 lines of 4096 samples), a causal plan: the step between two HIP
events and the kernels from the timed calls.  Byte model per sample: var2_biquad_tails_1d reads six signals and writes v, 24 + 4 B
(and 6 floats per tile and per group); var2_pass2_1d reads 12 B and writes 4 B; var2_biquad_grad_1d reads lam and the three taps
and writes grad_in, 20 B, with coefficient gradients reads x and y too and writes five more signals, 48 B.  The pass kernels' rates
are given as a fraction of rf_stream_copy's on a 4096 x 4096 plane (8 B per sample).  Beside them:
  (a) the all-pole step on the same signals (rf_var2_plan_execute);
  (b) the route a caller had: v = b0 * x + b1 * shift(x) + b2 * shift2(x) as a torch expression, then allpole_scan -- forward alone
      (no_grad) and forward plus backward through autograd with all six signals requiring gradients -- against biquad_scan, with
      the peak of torch's device memory above what the inputs hold for both (the plan's own adjoint-state signal is given beside)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

TILE, GROUP = 64, 64
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


def kernel_bytes(name, n, lines, coefficients):
    tiles = -(-n // TILE)
    groups = -(-tiles // GROUP)
    if "biquad_tails" in name:
        return lines * (28 * n + 4 * 6 * (tiles + groups))
    if "tails" in name:
        return lines * (12 * n + 4 * 6 * (tiles + groups))
    if "carry" in name:
        return lines * 4 * groups * (6 + 2)
    if "grad" in name:
        return lines * (48 if coefficients else 20) * n
    return lines * (16 * n + 4 * 6 * tiles + 4 * 2 * groups)


def torch_route(x, b0, b1, b2, a1, a2):
    """what a caller wrote before: the feed-forward half as a torch expression in front of allpole_scan"""
    import torch
    import recfilter_amd as rfa
    pad = torch.nn.functional.pad
    v = b0 * x + b1 * pad(x, (1, 0))[..., :-1] + b2 * pad(x, (2, 0))[..., :-2]
    return rfa.allpole_scan(v, a1, a2)


def peak_of(fn, prepare):
    """the peak of torch's allocated device memory above what was held before, in bytes, over one call of fn; prepare() drops what
    an earlier call left behind (the leaves' gradients), so the outputs and gradients of this call count"""
    import torch
    prepare()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def probe(n, lines, steps, rounds, copy_planes):
    import math
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(30)
    shape = (n,) if lines == 1 else (lines, n)
    rand = lambda: torch.rand(shape, device="cuda", generator=gen)
    x = rand() * 2 - 1
    theta, r = 0.2 + (math.pi - 0.4) * rand(), 0.5 + 0.48 * rand()
    a1, a2 = (-2 * r * torch.cos(theta)).contiguous(), (r * r).contiguous()
    phi, q, k = 0.2 + (math.pi - 0.4) * rand(), 0.3 + 0.7 * rand(), 0.5 + rand()
    b0, b1, b2 = k.contiguous(), (-2 * k * q * torch.cos(phi)).contiguous(), (k * q * q).contiguous()
    del theta, r, phi, q, k
    inputs = (x, b0, b1, b2, a1, a2)
    out, g, gin = torch.empty_like(x), rand() * 2 - 1, torch.empty_like(x)
    grads = tuple(torch.empty_like(x) for _ in range(5))
    leaves = [t.detach().requires_grad_() for t in inputs]

    def clear():
        for t in leaves:
            t.grad = None

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn(*inputs)
        return run

    def with_grad(fn):
        def run():
            clear()
            fn(*leaves).backward(g)
        return run
    say(f"== {n} samples x {lines} line(s)")
    with rfa.Var2Plan(n, lines=lines) as plan:
        runs = {"biquad": lambda: plan.execute_biquad(*inputs, out),
                "all-pole": lambda: plan.execute(x, a1, a2, out),
                "backward": lambda: plan.backward_biquad(*inputs, None, g, gin),
                "backward+coef": lambda: plan.backward_biquad(*inputs, out, g, gin, grads),
                "torch forward": no_grad(torch_route), "ours forward": no_grad(rfa.biquad_scan),
                "torch forward+backward": with_grad(torch_route), "ours forward+backward": with_grad(rfa.biquad_scan)}
        for _ in range(3):
            rfa.stream_copy_ms(*copy_planes, reps=2)
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        copy, step, kernels = [], {name: [] for name in runs}, {}
        for _ in range(rounds):
            copy.append(rfa.stream_copy_ms(*copy_planes, reps=steps))
            for name, fn in runs.items():
                step[name].append(timed(fn, steps))
            reports = ([("forward", *r) for r in plan.execute_biquad_timed(*inputs, out)[1]]
                       + [("backward", *r) for r in plan.backward_biquad_timed(*inputs, None, g, gin)[2]]
                       + [("backward+coef", *r) for r in plan.backward_biquad_timed(*inputs, out, g, gin, grads)[2]])
            for i, (stage, kname, ms) in enumerate(reports):
                kernels.setdefault((i, stage, kname), []).append(ms)
        clear()
        copy_rate = 8.0 * copy_planes[0].numel() / (med(copy) * 1e-3)
        say(f" - {plan.biquad_num_kernels} + {plan.backward_biquad_num_kernels} launches, workspace {plan.workspace_bytes / 2**20:.2f} MiB, "
            f"adjoint state {plan.backward_biquad_bytes / 2**20:.2f} MiB; rf_stream_copy {copy_rate / 1e12:.3f} TB/s {spread(copy)} ms")
        for (i, stage, kname), ms in sorted(kernels.items()):
            b = kernel_bytes(kname, n, lines, stage == "backward+coef")
            rate = b / (med(ms) * 1e-3)
            say(f"     {stage:<13} {kname:<21} {med(ms):9.4f} ms {spread(ms)}   {b / 2**20:10.2f} MiB   {rate / 1e12:6.3f} TB/s   {rate / copy_rate:5.2f} of the copy rate")
        fwd, pole = med(step["biquad"]), med(step["all-pole"])
        say(f"     step                         {fwd:9.4f} ms {spread(step['biquad'])}   {lines * n / fwd / 1e6:.1f} Gsamples/s")
        say(f"     (a) all-pole step            {pole:9.4f} ms {spread(step['all-pole'])}   biquad step / this {fwd / pole:.2f}")
        say(f"     backward                     {med(step['backward']):9.4f} ms {spread(step['backward'])}   {med(step['backward']) / fwd:.2f} forward steps")
        say(f"     backward, coefficients too   {med(step['backward+coef']):9.4f} ms {spread(step['backward+coef'])}   {med(step['backward+coef']) / fwd:.2f} forward steps")
        peaks = {name: peak_of(runs[name], clear) for name in ("torch forward", "ours forward", "torch forward+backward", "ours forward+backward")}
        clear()
        for what in ("forward", "forward+backward"):
            t, o = med(step[f"torch {what}"]), med(step[f"ours {what}"])
            say(f"     (b) {what:<17} torch expression + allpole_scan {t:9.4f} ms {spread(step[f'torch {what}'])}, peak {peaks[f'torch {what}'] / 2**20:.1f} MiB;"
                f"  biquad_scan {o:9.4f} ms {spread(step[f'ours {what}'])}, peak {peaks[f'ours {what}'] / 2**20:.1f} MiB;  torch / ours {t / o:.2f} in time, "
                f"{peaks[f'torch {what}'] / max(peaks[f'ours {what}'], 1):.2f} in memory")
    del x, a1, a2, b0, b1, b2, out, g, gin, grads, leaves, inputs
    torch.cuda.empty_cache()


def main():
    global out_file
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="+", default=["10000000:1", f"{1 << 24}:1", f"{1 << 28}:1", "4096:4096"], help="LENGTH:LINES")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("biquad_probe: needs a GPU")
    if a.out:
        out_file = open(a.out, "w")
    say(f"biquad_probe: {torch.cuda.get_device_name(0)}; steps {a.steps}, rounds {a.rounds}; medians over the rounds (min, max)")
    copy_planes = (torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda"))
    for case in a.cases:
        n, lines = (int(v) for v in case.split(":"))
        probe(n, lines, a.steps, a.rounds, copy_planes)
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
