#!/usr/bin/env python3
"""The direct-form-I section on control-rate frames (rf_var2_plan_execute_biquad_frames / _backward_biquad_frames,
kernels_var2_signal.hip): whole-step and per-kernel times beside the measured copy rate, the section on signals expanded beforehand
and the route a caller had before, everything alternating in ONE process (the protocol of var2_probe.py: medians of `rounds` rounds
of `steps` steps, with the rounds' min and max).

    python tools/probes/var2_frames_probe.py [--cases N:LINES ...] [--hops 64 512 4096] [--steps 10] [--rounds 5] [--out FILE]

Per case (default: 10^7, 2^24 and 2^28 samples on one line, 4096 lines of 4096 samples) and hop, a causal plan.  Byte model per
sample: var2_biquad_frames_tails_1d reads x and writes v, 8 B (and 6 floats per tile and per group); var2_frames_pass2_1d 8 B;
var2_adj_frames_tails_1d 4 B, var2_adj_frames_pass2_1d 8 B; var2_biquad_frames_grad_1d reads lam and writes grad_in, 8 B, with frame
gradients reads x and y too, 16 B, and writes 80 B per piece of min(hop, 1024) samples, which var2_frames_fold_1d reads.  The
frames themselves are 20 F / N B per sample.  The kernels' rates are given as a fraction of rf_stream_copy's on a 4096 x 4096
plane (8 B per sample).  Beside them:
  (a) execute_biquad / backward_biquad with all five coefficient gradients, alone, on signals expanded beforehand (44 B and 76 B);
  (b) the route a caller had: torch.lerp of the five frame tensors up to audio rate, then biquad_scan -- forward alone (no_grad)
      and forward plus backward through autograd with x and the five frame tensors requiring gradients -- against
      biquad_scan_frames, with the peak of torch's device memory above what the inputs hold for both."""
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


def kernel_bytes(name, n, lines, hop, with_frames):
    tiles = -(-n // TILE)
    groups = -(-tiles // GROUP)
    pieces = -(-n // min(hop, 1024))
    count = -(-n // hop) + 1
    if "fold" in name:
        return lines * (80 * pieces + 20 * count)
    if "grad" in name:
        return lines * ((16 * n + 80 * pieces) if with_frames else 8 * n)
    if "adj_frames_tails" in name:
        return lines * (4 * n + 4 * 6 * (tiles + groups))
    if "tails" in name:
        return lines * (8 * n + 4 * 6 * (tiles + groups))
    if "carry" in name:
        return lines * 4 * groups * (6 + 2)
    return lines * (8 * n + 4 * 6 * tiles + 4 * 2 * groups)


def lerp_route(n, hop):
    """what a caller wrote before: every frame tensor interpolated up to audio rate, then the section on signals"""
    import torch
    import recfilter_amd as rfa
    w = (torch.arange(hop, device="cuda", dtype=torch.float32) / hop)

    def expanded(f):
        return torch.lerp(f[..., :-1, None], f[..., 1:, None], w).flatten(-2)[..., :n]

    def run(x, *frames):
        return rfa.biquad_scan(x, *(expanded(f) for f in frames))
    return run


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


def probe(n, lines, hop, steps, rounds, copy_planes):
    import math
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(33)
    count = rfa.frames_count(n, hop)
    shape, fshape = ((n,), (count,)) if lines == 1 else ((lines, n), (lines, count))
    rand = lambda s: torch.rand(s, device="cuda", generator=gen)      # noqa: E731
    x, g = rand(shape) * 2 - 1, rand(shape) * 2 - 1
    theta, r = 0.2 + (math.pi - 0.4) * rand(fshape), 0.5 + 0.48 * rand(fshape)
    phi, q, k = 0.2 + (math.pi - 0.4) * rand(fshape), 0.3 + 0.7 * rand(fshape), 0.5 + rand(fshape)
    frames = tuple(t.contiguous() for t in (k, -2 * k * q * torch.cos(phi), k * q * q, -2 * r * torch.cos(theta), r * r))
    signals = tuple(rfa.expand_frames(f, hop, n) for f in frames)
    out, gin = torch.empty_like(x), torch.empty_like(x)
    fgrads = tuple(torch.empty_like(f) for f in frames)
    sgrads = tuple(torch.empty_like(x) for _ in range(5))
    leaves = [t.detach().requires_grad_() for t in (x,) + frames]
    old = lerp_route(n, hop)
    new = lambda xx, *ff: rfa.biquad_scan_frames(xx, *ff, hop)      # noqa: E731

    def clear():
        for t in leaves:
            t.grad = None

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn(x, *frames)
        return run

    def with_grad(fn):
        def run():
            clear()
            fn(*leaves).backward(g)
        return run
    say(f"== {n} samples x {lines} line(s), hop {hop}: {count} frames per coefficient and line")
    with rfa.Var2Plan(n, lines=lines) as plan:
        runs = {"frames": lambda: plan.execute_biquad_frames(x, frames, hop, out),
                "signals": lambda: plan.execute_biquad(x, *signals, out),
                "frames backward": lambda: plan.backward_biquad_frames(x, frames, hop, None, g, gin),
                "frames backward+grads": lambda: plan.backward_biquad_frames(x, frames, hop, out, g, gin, fgrads),
                "signals backward+grads": lambda: plan.backward_biquad(x, *signals, out, g, gin, sgrads),
                "lerp forward": no_grad(old), "frames forward": no_grad(new),
                "lerp forward+backward": with_grad(old), "frames forward+backward": with_grad(new)}
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
            reports = ([("forward", *t) for t in plan.execute_biquad_frames_timed(x, frames, hop, out)[1]]
                       + [("backward", *t) for t in plan.backward_biquad_frames_timed(x, frames, hop, None, g, gin)[2]]
                       + [("backward+grads", *t) for t in plan.backward_biquad_frames_timed(x, frames, hop, out, g, gin, fgrads)[2]])
            for i, (stage, kname, ms) in enumerate(reports):
                kernels.setdefault((i, stage, kname), []).append(ms)
        clear()
        copy_rate = 8.0 * copy_planes[0].numel() / (med(copy) * 1e-3)
        say(f" - {plan.biquad_frames_num_kernels} + {plan.backward_biquad_frames_num_kernels(False)} / {plan.backward_biquad_frames_num_kernels(True)} launches, "
            f"workspace {plan.workspace_bytes / 2**20:.2f} MiB, adjoint state and slab {plan.backward_biquad_frames_bytes(hop) / 2**20:.2f} MiB; "
            f"rf_stream_copy {copy_rate / 1e12:.3f} TB/s {spread(copy)} ms")
        for (i, stage, kname), ms in sorted(kernels.items()):
            b = kernel_bytes(kname, n, lines, hop, stage == "backward+grads")
            rate = b / (med(ms) * 1e-3)
            say(f"     {stage:<14} {kname:<28} {med(ms):9.4f} ms {spread(ms)}   {b / 2**20:10.2f} MiB   {rate / 1e12:6.3f} TB/s   {rate / copy_rate:5.2f} of the copy rate")
        fwd, sig = med(step["frames"]), med(step["signals"])
        both = fwd + med(step["frames backward+grads"])
        sig_both = sig + med(step["signals backward+grads"])
        say(f"     step, frames                    {fwd:9.4f} ms {spread(step['frames'])}   {lines * n / fwd / 1e6:.1f} Gsamples/s")
        say(f"     (a) step, expanded signals      {sig:9.4f} ms {spread(step['signals'])}   frames / signals {fwd / sig:.2f}   (byte model 16 / 44 = 0.36)")
        say(f"     backward, frames                {med(step['frames backward']):9.4f} ms {spread(step['frames backward'])}")
        say(f"     backward with frame gradients   {med(step['frames backward+grads']):9.4f} ms {spread(step['frames backward+grads'])}")
        say(f"     (a) backward with coefficient gradients, expanded signals {med(step['signals backward+grads']):9.4f} ms {spread(step['signals backward+grads'])}"
            f"   frames / signals {med(step['frames backward+grads']) / med(step['signals backward+grads']):.2f}   (byte model 28 / 76 = 0.37)")
        say(f"     (a) forward + backward with gradients: frames {both:9.4f} ms, expanded signals {sig_both:9.4f} ms, frames / signals {both / sig_both:.2f}")
        names = ("lerp forward", "frames forward", "lerp forward+backward", "frames forward+backward")
        peaks = {name: peak_of(runs[name], clear) for name in names}
        clear()
        for what in ("forward", "forward+backward"):
            t, o = med(step[f"lerp {what}"]), med(step[f"frames {what}"])
            say(f"     (b) {what:<17} torch.lerp + biquad_scan {t:9.4f} ms {spread(step[f'lerp {what}'])}, peak {peaks[f'lerp {what}'] / 2**20:.1f} MiB;"
                f"  biquad_scan_frames {o:9.4f} ms {spread(step[f'frames {what}'])}, peak {peaks[f'frames {what}'] / 2**20:.1f} MiB;  frames / lerp {o / t:.2f} in time, "
                f"{peaks[f'frames {what}'] / max(peaks[f'lerp {what}'], 1):.2f} in memory")
    del x, g, frames, signals, out, gin, fgrads, sgrads, leaves
    torch.cuda.empty_cache()


def main():
    global out_file
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="+", default=["10000000:1", f"{1 << 24}:1", f"{1 << 28}:1", "4096:4096"], help="LENGTH:LINES")
    ap.add_argument("--hops", nargs="+", type=int, default=[64, 512, 4096])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("var2_frames_probe: needs a GPU")
    if a.out:
        out_file = open(a.out, "w")
    say(f"var2_frames_probe: {torch.cuda.get_device_name(0)}; steps {a.steps}, rounds {a.rounds}; medians over the rounds (min, max)")
    copy_planes = (torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda"))
    for case in a.cases:
        n, lines = (int(v) for v in case.split(":"))
        for hop in a.hops:
            probe(n, lines, hop, a.steps, a.rounds, copy_planes)
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
