#!/usr/bin/env python3
"""Time-varying second-order all-pole scans on signals (rf_var2_plan_*, kernels_var2_signal.hip): whole-step and per-kernel times
beside the measured copy rate and beside the plans a caller had before, everything alternating in ONE process (the protocol of
var_probe.py: medians of `rounds` rounds of `steps` steps, with the rounds' min and max).

    python tools/probes/var2_probe.py [--cases N:LINES ...] [--steps 10] [--rounds 5] [--out FILE]

Per case (default: 10^7, 2^24 and 2^28 samples on one line, 4096 lines of 4096 samples), a causal plan: the step between two HIP
events and the three kernels from execute_timed.  Byte model: var2_tails_1d reads the three signals, 12 B per sample, and writes 6
floats per tile and per group; var2_pass2_1d reads 12 B and writes 4 B per sample and reads the maps; var2_carry_1d moves the
groups' aggregates and carries only.  The two pass kernels' rates are given as a fraction of rf_stream_copy's on a 4096 x 4096 plane
(8 B per sample).  Beside them, none of it the code under test:
  (a) the first-order varying signal plan's +x step on the same length (rf_var_plan_create_signal; one weight signal: 8 and 12 B
      per sample in its two passes) -- per line where there are several, the lines as its planes are not comparable (they would share
      the weights), so it is given for one line only;
  (b) rf_plan's order-2 causal scan with constant coefficients on the same signal, one line only.
And the backward, without and with the coefficient gradients, in forward steps."""
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


def kernel_bytes(name, n, lines):
    tiles = -(-n // TILE)
    groups = -(-tiles // GROUP)
    if "tails" in name:
        return lines * (12 * n + 4 * 6 * (tiles + groups))
    if "carry" in name:
        return lines * 4 * groups * (6 + 2)
    if "grad" in name:
        return lines * 16 * n
    return lines * (16 * n + 4 * 6 * tiles + 4 * 2 * groups)


def probe(n, lines, steps, rounds, copy_planes):
    import math
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(29)
    shape = (n,) if lines == 1 else (lines, n)
    x = torch.rand(shape, device="cuda", generator=gen) * 2 - 1
    theta = 0.2 + (math.pi - 0.4) * torch.rand(shape, device="cuda", generator=gen)
    r = 0.5 + 0.48 * torch.rand(shape, device="cuda", generator=gen)
    a1 = (-2 * r * torch.cos(theta)).contiguous()
    a2 = (r * r).contiguous()
    del theta, r
    out, g = torch.empty_like(x), torch.rand(shape, device="cuda", generator=gen) * 2 - 1
    gin, g1, g2 = (torch.empty_like(x) for _ in range(3))
    say(f"== {n} samples x {lines} line(s)")
    with rfa.Var2Plan(n, lines=lines) as plan:
        runs = {"var2": lambda: plan.execute(x, a1, a2, out),
                "backward": lambda: plan.backward(a1, a2, None, g, gin),
                "backward+coef": lambda: plan.backward(a1, a2, out, g, gin, g1, g2)}
        others = []
        if lines == 1:
            first = rfa.VarPlan.signal(n, [(0, True, 0)])
            const = rfa.Plan((n,), [(0, True, [1.0, 1.2, -0.5])], flags=0)
            w = torch.rand(n, device="cuda", generator=gen)
            runs["first order +x"] = lambda: first.execute([x], [w], [out])
            runs["constant order 2"] = lambda: const.execute([x], [out])
            others = [first, const]
        for _ in range(3):
            rfa.stream_copy_ms(*copy_planes, reps=2)
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        copy, step, kernels = [], {k: [] for k in runs}, {}
        for _ in range(rounds):
            copy.append(rfa.stream_copy_ms(*copy_planes, reps=steps))
            for k, fn in runs.items():
                step[k].append(timed(fn, steps))
            reports = plan.execute_timed(x, a1, a2, out)[1] + plan.backward_timed(a1, a2, out, g, gin, g1, g2)[3]
            for i, (kname, ms) in enumerate(reports):
                kernels.setdefault((i, kname), []).append(ms)
        copy_rate = 8.0 * copy_planes[0].numel() / (med(copy) * 1e-3)
        say(f" - {plan.num_kernels} launches, workspace {plan.workspace_bytes / 2**20:.2f} MiB; rf_stream_copy {copy_rate / 1e12:.3f} TB/s {spread(copy)} ms")
        for (i, kname), ms in sorted(kernels.items()):
            b = kernel_bytes(kname, n, lines)
            rate = b / (med(ms) * 1e-3)
            say(f"     {'forward' if i < 3 else 'backward':<8} {kname:<18} {med(ms):9.4f} ms {spread(ms)}   {b / 2**20:10.2f} MiB   {rate / 1e12:6.3f} TB/s   {rate / copy_rate:5.2f} of the copy rate")
        fwd = med(step["var2"])
        say(f"     step                        {fwd:9.4f} ms {spread(step['var2'])}   {lines * n / fwd / 1e6:.1f} Gsamples/s")
        say(f"     backward                    {med(step['backward']):9.4f} ms {spread(step['backward'])}   {med(step['backward']) / fwd:.2f} forward steps")
        say(f"     backward, coefficients too  {med(step['backward+coef']):9.4f} ms {spread(step['backward+coef'])}   {med(step['backward+coef']) / fwd:.2f} forward steps")
        if lines == 1:
            for k, label in (("first order +x", "(a) first-order varying +x step"), ("constant order 2", f"(b) rf_plan order 2, constant ({others[1].path_name})")):
                say(f"     {label:<40} {med(step[k]):9.4f} ms {spread(step[k])}   var2 step / this {fwd / med(step[k]):.2f}")
        for p in others:
            p.close()
    del x, a1, a2, out, g, gin, g1, g2
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
        sys.exit("var2_probe: needs a GPU")
    if a.out:
        out_file = open(a.out, "w")
    say(f"var2_probe: {torch.cuda.get_device_name(0)}; steps {a.steps}, rounds {a.rounds}; medians over the rounds (min, max)")
    copy_planes = (torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda"))
    for case in a.cases:
        n, lines = (int(v) for v in case.split(":"))
        probe(n, lines, a.steps, a.rounds, copy_planes)
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
