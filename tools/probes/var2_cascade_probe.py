#!/usr/bin/env python3
"""Cascades of time-varying direct-form-I sections on signals (rf_var2_plan_execute_cascade / _backward_cascade, var2_link_1d of
kernels_var2_signal.hip): whole-step and per-kernel times beside the measured copy rate and beside the route a caller had, K
separate sections, everything alternating in ONE process (the protocol of biquad_probe.py: medians of `rounds` rounds of `steps`
steps, with the rounds' min and max).

    python tools/probes/var2_cascade_probe.py [--cases N:LINES ...] [--sections 2 4 8] [--steps 10] [--rounds 5] [--out FILE]

Per case (default: 10^7, 2^24 and 2^28 samples on one line, 4096 lines of 4096 samples) and per K, a causal plan; the sections
share ONE set of five coefficient signals, to bound the memory.  Byte model per sample: var2_biquad_tails_1d 24 + 4 B, var2_link_1d
reads v, two feedback coefficients and the next section's five and writes v, 32 + 4 B (var2_link_keep_1d 4 more), var2_pass2_1d
12 + 4 B: a forward step moves 36 K + 8 B against 44 K of K separate sections.  The kernels' rates are given as a fraction of
rf_stream_copy's on a 4096 x 4096 plane (8 B per sample).  Beside the step:
  (a) K execute_biquad calls ping-ponging two buffers;
  (b) forward plus backward through biquad_cascade against K chained biquad_scan calls under autograd, all signals requiring
      gradients, with the peak of torch's device memory above what the inputs hold for both and the plan's own bytes beside;
  (c) up to 2^25 samples, the memory of (b) with coefficient signals of its own for every section."""
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
    """the forward's kernels under the byte model"""
    tiles = -(-n // TILE)
    groups = -(-tiles // GROUP)
    slots = 4 * 6 * (tiles + groups)
    if "biquad_tails" in name:
        return lines * (28 * n + slots)
    if "link" in name:
        return lines * ((40 if "keep" in name else 36) * n + slots + 4 * 6 * tiles + 4 * 2 * groups)
    if "carry" in name:
        return lines * 4 * groups * (6 + 2)
    return lines * (16 * n + 4 * 6 * tiles + 4 * 2 * groups)


def peak_of(fn, prepare):
    """the peak of torch's allocated device memory above what was held before, in bytes, over one call of fn"""
    import torch
    prepare()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def probe(n, lines, counts, steps, rounds, copy_planes):
    import math
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(31)
    shape = (n,) if lines == 1 else (lines, n)
    rand = lambda: torch.rand(shape, device="cuda", generator=gen)      # noqa: E731
    x = rand() * 2 - 1
    theta, r = 0.2 + (math.pi - 0.4) * rand(), 0.5 + 0.48 * rand()
    a1, a2 = (-2 * r * torch.cos(theta)).contiguous(), (r * r).contiguous()
    phi, q, k = 0.2 + (math.pi - 0.4) * rand(), 0.3 + 0.7 * rand(), 0.5 + 0.5 * rand()
    b0, b1, b2 = k.contiguous(), (-2 * k * q * torch.cos(phi)).contiguous(), (k * q * q).contiguous()
    del theta, r, phi, q, k
    section = (b0, b1, b2, a1, a2)
    out, other, g = torch.empty_like(x), torch.empty_like(x), rand() * 2 - 1
    leaves = [t.detach().requires_grad_() for t in (x,) + section]

    def clear():
        for t in leaves:
            t.grad = None
    say(f"== {n} samples x {lines} line(s)")
    with rfa.Var2Plan(n, lines=lines) as plan:
        for K in counts:
            sections = [section] * K

            def separate():
                src = x
                for i in range(K):
                    dst = out if (K - 1 - i) % 2 == 0 else other
                    plan.execute_biquad(src, *section, dst)
                    src = dst

            def fused_autograd():
                clear()
                rfa.biquad_cascade(leaves[0], [tuple(leaves[1:])] * K).backward(g)

            def chained_autograd():
                clear()
                t = leaves[0]
                for _ in range(K):
                    t = rfa.biquad_scan(t, *leaves[1:])
                t.backward(g)
            runs = {"cascade": lambda: plan.execute_cascade(x, sections, out), "separate": separate,
                    "cascade forward+backward": fused_autograd, "chained forward+backward": chained_autograd}
            for _ in range(2):
                rfa.stream_copy_ms(*copy_planes, reps=2)
                for fn in runs.values():
                    fn()
            torch.cuda.synchronize()
            copy, step, kernels = [], {name: [] for name in runs}, {}
            for _ in range(rounds):
                copy.append(rfa.stream_copy_ms(*copy_planes, reps=steps))
                for name, fn in runs.items():
                    step[name].append(timed(fn, steps))
                for i, (kname, ms) in enumerate(plan.execute_cascade_timed(x, sections, out)[1]):
                    # the first launch, the carries and the links between sections (every launch of every round in one list),
                    # the last carry, the last pass
                    place = 0 if i == 0 else (3 + i - (2 * K - 1) if i >= 2 * K - 1 else 2 - i % 2)
                    kernels.setdefault((place, kname), []).append(ms)
            clear()
            copy_rate = 8.0 * copy_planes[0].numel() / (med(copy) * 1e-3)
            say(f" - K = {K}: {plan.cascade_num_kernels(K)} + {plan.backward_cascade_num_kernels(K)} launches, workspace {plan.workspace_bytes / 2**20:.2f} MiB, "
                f"the backward's signals {plan.backward_cascade_bytes(K) / 2**20:.2f} MiB; rf_stream_copy {copy_rate / 1e12:.3f} TB/s {spread(copy)} ms")
            for (i, kname), ms in sorted(kernels.items()):
                b = kernel_bytes(kname, n, lines)
                rate = b / (med(ms) * 1e-3)
                say(f"     {kname:<21} {med(ms):9.4f} ms {spread(ms)}   {b / 2**20:10.2f} MiB   {rate / 1e12:6.3f} TB/s   {rate / copy_rate:5.2f} of the copy rate"
                    + (f"   (median of the {K - 1} between sections)" if i in (1, 2) and K > 2 else ""))
            fused, sep = med(step["cascade"]), med(step["separate"])
            say(f"     step                         {fused:9.4f} ms {spread(step['cascade'])}   {lines * n * K / fused / 1e6:.1f} Gsample-sections/s")
            say(f"     (a) {K} execute_biquad calls   {sep:9.4f} ms {spread(step['separate'])}   cascade / separate {fused / sep:.3f}   (byte model {(36 * K + 8) / (44 * K):.3f})")
            peaks = {name: peak_of(runs[name], clear) for name in ("cascade forward+backward", "chained forward+backward")}
            clear()
            f, c = med(step["cascade forward+backward"]), med(step["chained forward+backward"])
            say(f"     (b) forward+backward   biquad_cascade {f:9.4f} ms {spread(step['cascade forward+backward'])}, peak {peaks['cascade forward+backward'] / 2**20:.1f} MiB "
                f"(+ the plan's {plan.backward_cascade_bytes(K) / 2**20:.1f} MiB);  {K} chained biquad_scan {c:9.4f} ms {spread(step['chained forward+backward'])}, "
                f"peak {peaks['chained forward+backward'] / 2**20:.1f} MiB (+ the plan's {plan.backward_biquad_bytes / 2**20:.1f} MiB);  cascade / chained {f / c:.3f} in time")
            if lines * n <= 1 << 25:
                # (c) the memory of (b) again with coefficient signals of its own for every section, as a caller has them: the
                # shared leaves above let autograd fold a chained section's gradients away before the next section's are formed
                own = [[t.detach().clone().requires_grad_() for t in section] for _ in range(K)]
                xl = leaves[0]

                def drop():
                    xl.grad = None
                    for s in own:
                        for t in s:
                            t.grad = None

                def fused_own():
                    rfa.biquad_cascade(xl, own).backward(g)

                def chained_own():
                    t = xl
                    for s in own:
                        t = rfa.biquad_scan(t, *s)
                    t.backward(g)
                pf, pc = peak_of(fused_own, drop), peak_of(chained_own, drop)
                drop()
                span = 4 * lines * n / 2**20
                say(f"     (c) coefficient signals of its own per section ({5 * K} leaves): peak biquad_cascade {pf / 2**20:.1f} MiB = {pf / 2**20 / span:.0f} signals "
                    f"(+ the plan's {K + 1});  chained {pc / 2**20:.1f} MiB = {pc / 2**20 / span:.0f} signals (+ the plan's 1)")
                del own
    del x, a1, a2, b0, b1, b2, out, other, g, leaves, section
    torch.cuda.empty_cache()


def main():
    global out_file
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="+", default=["10000000:1", f"{1 << 24}:1", f"{1 << 28}:1", "4096:4096"], help="LENGTH:LINES")
    ap.add_argument("--sections", nargs="+", type=int, default=[2, 4, 8])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("var2_cascade_probe: needs a GPU")
    if a.out:
        out_file = open(a.out, "w")
    say(f"var2_cascade_probe: {torch.cuda.get_device_name(0)}; steps {a.steps}, rounds {a.rounds}; medians over the rounds (min, max)")
    copy_planes = (torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda"))
    for case in a.cases:
        n, lines = (int(v) for v in case.split(":"))
        probe(n, lines, a.sections, a.steps, a.rounds, copy_planes)
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
