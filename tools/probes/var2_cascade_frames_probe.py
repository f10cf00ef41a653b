#!/usr/bin/env python3
"""Cascades on control-rate frames (rf_var2_plan_execute_cascade_frames / _backward_cascade_frames, kernels_var2_signal.hip):
whole-step and per-kernel times beside the measured copy rate and the routes a caller had before, everything alternating in ONE
process (the protocol of var2_probe.py: medians of `rounds` rounds of `steps` steps, with the rounds' min and max).

    python tools/probes/var2_cascade_frames_probe.py [--cases N:LINES ...] [--hops 64 512 4096] [--sections 2 4 8] [--steps 10]
                                                     [--rounds 5] [--out FILE]

Per case (default: 10^7, 2^24 and 2^28 samples on one line, 4096 lines of 4096 samples), hop and K, a causal plan.  Byte model per
sample: var2_biquad_frames_tails_1d, var2_frames_link_1d, var2_frames_pass2_1d and their adjoint counterparts read 4 B and write
4 B (the adjoint tails stage reads 4 B alone; a keep link writes 4 B more); var2_frames_coef_1d reads lam, x and y, 12 B, and
writes 80 B per piece of min(hop, 1024) samples; var2_biquad_frames_grad_1d 8 B, with frame gradients 16 B and the pieces;
var2_frames_fold_cascade_1d reads the K slabs.  The kernels' rates are given as a fraction of rf_stream_copy's on a 4096 x 4096
plane (8 B per sample).  Beside the new calls:
  (a) K execute_biquad_frames calls ping-ponging two buffers (16 K B per sample against 8 K + 8), and K chained
      backward_biquad_frames calls (28 K with frame gradients against 24 K + 4; 16 K without against 8 K + 4);
  (b) execute_cascade on signals expanded beforehand (36 K + 8 B);
  (c) a training step through K chained biquad_scan_frames against biquad_cascade_frames, x and all 5 K frame tensors requiring
      gradients, with the peak of torch's device memory above what the inputs hold;
  (d) the same through torch.lerp of every frame tensor up to audio rate and biquad_cascade(keep=True)."""
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


def kernel_bytes(name, n, lines, hop, K):
    tiles = -(-n // TILE)
    groups = -(-tiles // GROUP)
    pieces = -(-n // min(hop, 1024))
    count = -(-n // hop) + 1
    maps = 4 * 6 * (tiles + groups)
    if "fold" in name:
        return lines * K * (80 * pieces + 20 * count)
    if "coef" in name:
        return lines * (12 * n + 80 * pieces)
    if "grad" in name:
        return lines * (16 * n + 80 * pieces)      # (8 n without frame gradients: reported under its own stage)
    if "carry" in name:
        return lines * 4 * groups * (6 + 2)
    if "link_keep" in name:
        return lines * (12 * n + 2 * maps)
    if "link" in name:
        return lines * (8 * n + 2 * maps)
    if "adj_frames_tails" in name:
        return lines * (4 * n + maps)
    return lines * (8 * n + maps)


def lerp_route(n, hop):
    """what a caller wrote before: every frame tensor interpolated up to audio rate, then the cascade on signals, keeping"""
    import torch
    import recfilter_amd as rfa
    w = (torch.arange(hop, device="cuda", dtype=torch.float32) / hop)

    def expanded(f):
        return torch.lerp(f[..., :-1, None], f[..., 1:, None], w).flatten(-2)[..., :n]

    def run(x, sections):
        return rfa.biquad_cascade(x, [tuple(expanded(f) for f in s) for s in sections], keep=True)
    return run


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


def probe(n, lines, hop, K, steps, rounds, copy_planes, with_signals):
    import math
    import torch
    import recfilter_amd as rfa
    gen = torch.Generator(device="cuda").manual_seed(34)
    count = rfa.frames_count(n, hop)
    shape, fshape = ((n,), (count,)) if lines == 1 else ((lines, n), (lines, count))
    rand = lambda s: torch.rand(s, device="cuda", generator=gen)      # noqa: E731
    x, g = rand(shape) * 2 - 1, rand(shape) * 2 - 1

    def section():
        theta, r = 0.2 + (math.pi - 0.4) * rand(fshape), 0.5 + 0.48 * rand(fshape)
        phi, q, k = 0.2 + (math.pi - 0.4) * rand(fshape), 0.3 + 0.7 * rand(fshape), 0.5 + 0.5 * rand(fshape)
        return tuple(t.contiguous() for t in (k, -2 * k * q * torch.cos(phi), k * q * q, -2 * r * torch.cos(theta), r * r))
    sections = [section() for _ in range(K)]
    out, other, gin = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    kept = [torch.empty_like(x) for _ in range(K - 1)]
    fgrads = [tuple(torch.empty_like(f) for f in s) for s in sections]
    leaves = [x.detach().requires_grad_()] + [f.detach().requires_grad_() for s in sections for f in s]
    leaf_sections = [tuple(leaves[1 + 5 * k:6 + 5 * k]) for k in range(K)]
    say(f"== {n} samples x {lines} line(s), hop {hop}, K = {K}: {count} frames per coefficient and line")
    with rfa.Var2Plan(n, lines=lines) as plan:
        def chained_forward():
            src, dst = x, out if K % 2 == 1 else other      # the last call lands in `out`
            for s in sections:
                plan.execute_biquad_frames(src, s, hop, dst)
                src, dst = dst, (other if dst is out else out)

        def chained_backward(with_frames):
            results = [x] + kept + [out]      # (the values do not matter to the time: K + 1 signals of the right size)
            def run():
                src = g
                for k in range(K - 1, -1, -1):
                    plan.backward_biquad_frames(results[k], sections[k], hop, results[k + 1] if with_frames else None, src, gin if k % 2 == 0 else other,
                                                fgrads[k] if with_frames else None)
                    src = gin if k % 2 == 0 else other
            return run

        def clear():
            for t in leaves:
                t.grad = None

        def training(fn):
            def run():
                clear()
                fn(leaves[0], leaf_sections).backward(g)
            return run

        def chained_scans(xx, ss):
            for s in ss:
                xx = rfa.biquad_scan_frames(xx, *s, hop)
            return xx
        runs = {"cascade": lambda: plan.execute_cascade_frames(x, sections, hop, out),
                "cascade keep": lambda: plan.execute_cascade_frames(x, sections, hop, out, kept=kept),
                "chained": chained_forward,
                "cascade backward": lambda: plan.backward_cascade_frames(None, sections, hop, None, None, g, gin),
                "cascade backward+grads": lambda: plan.backward_cascade_frames(x, sections, hop, kept, out, g, gin, fgrads),
                "chained backward": chained_backward(False), "chained backward+grads": chained_backward(True),
                "cascade training": training(lambda xx, ss: rfa.biquad_cascade_frames(xx, ss, hop)),
                "chained training": training(chained_scans)}
        signals = None
        if with_signals:
            signals = [tuple(rfa.expand_frames(f, hop, n) for f in s) for s in sections]
            runs["signals"] = lambda: plan.execute_cascade(x, signals, out)
            runs["lerp training"] = training(lerp_route(n, hop))
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
            reports = ([("forward", *t) for t in plan.execute_cascade_frames_timed(x, sections, hop, out)[1]]
                       + [("forward keep", *t) for t in plan.execute_cascade_frames_timed(x, sections, hop, out, kept=kept)[2]]
                       + [("backward", *t) for t in plan.backward_cascade_frames_timed(None, sections, hop, None, None, g, gin)[2]]
                       + [("backward+grads", *t) for t in plan.backward_cascade_frames_timed(x, sections, hop, kept, out, g, gin, fgrads)[2]])
            seen = {}
            for stage, kname, ms in reports:      # the launches of one name in one stage: their sum
                seen[stage, kname] = seen.get((stage, kname), 0.0) + ms
            for key, ms in seen.items():
                kernels.setdefault(key, []).append(ms)
        clear()
        copy_rate = 8.0 * copy_planes[0].numel() / (med(copy) * 1e-3)
        say(f" - {plan.cascade_frames_num_kernels(K)} + {plan.backward_cascade_frames_num_kernels(K, False)} / {plan.backward_cascade_frames_num_kernels(K, True)} launches, "
            f"workspace {plan.workspace_bytes / 2**20:.2f} MiB, the plan's signals and slab {plan.backward_cascade_frames_bytes(K, hop) / 2**20:.2f} MiB; "
            f"rf_stream_copy {copy_rate / 1e12:.3f} TB/s {spread(copy)} ms")
        for (stage, kname), ms in kernels.items():
            launches = K - 1 if ("link" in kname or "coef" in kname) else K if "carry" in kname else 1
            b = kernel_bytes(kname, n, lines, hop, K) * launches
            if stage == "backward" and "grad" in kname:
                b = lines * 8 * n
            rate = b / (med(ms) * 1e-3)
            say(f"     {stage:<14} {launches:2d} x {kname:<30} {med(ms):9.4f} ms {spread(ms)}   {b / 2**20:10.2f} MiB   {rate / 1e12:6.3f} TB/s   {rate / copy_rate:5.2f} of the copy rate")
        m = {name: med(v) for name, v in step.items()}
        say(f"     forward, cascade on frames      {m['cascade']:9.4f} ms {spread(step['cascade'])}   {lines * n / m['cascade'] / 1e6:.1f} Gsamples/s; keeping {m['cascade keep']:9.4f} ms {spread(step['cascade keep'])}")
        say(f"     (a) K execute_biquad_frames     {m['chained']:9.4f} ms {spread(step['chained'])}   cascade / chained {m['cascade'] / m['chained']:.2f}   (byte model {(8 * K + 8) / (16 * K):.2f})")
        if with_signals:
            say(f"     (b) execute_cascade, expanded   {m['signals']:9.4f} ms {spread(step['signals'])}   cascade / signals {m['cascade'] / m['signals']:.2f}   (byte model {(8 * K + 8) / (36 * K + 8):.2f})")
        say(f"     backward, cascade on frames     {m['cascade backward']:9.4f} ms {spread(step['cascade backward'])};  (a) K backward_biquad_frames {m['chained backward']:9.4f} ms "
            f"{spread(step['chained backward'])}   cascade / chained {m['cascade backward'] / m['chained backward']:.2f}   (byte model {(8 * K + 4) / (16 * K):.2f})")
        say(f"     backward with frame gradients   {m['cascade backward+grads']:9.4f} ms {spread(step['cascade backward+grads'])};  (a) K backward_biquad_frames {m['chained backward+grads']:9.4f} ms "
            f"{spread(step['chained backward+grads'])}   cascade / chained {m['cascade backward+grads'] / m['chained backward+grads']:.2f}   (byte model {(24 * K + 4) / (28 * K):.2f})")
        names = ["cascade training", "chained training"] + (["lerp training"] if with_signals else [])
        peaks = {name: peak_of(runs[name], clear) for name in names}
        clear()
        say(f"     (c) training step: biquad_cascade_frames {m['cascade training']:9.4f} ms {spread(step['cascade training'])}, peak {peaks['cascade training'] / 2**20:.1f} MiB;  "
            f"K biquad_scan_frames {m['chained training']:9.4f} ms {spread(step['chained training'])}, peak {peaks['chained training'] / 2**20:.1f} MiB;  "
            f"cascade / chained {m['cascade training'] / m['chained training']:.2f} in time, {peaks['cascade training'] / max(peaks['chained training'], 1):.2f} in memory")
        if with_signals:
            say(f"     (d) training step: torch.lerp + biquad_cascade(keep=True) {m['lerp training']:9.4f} ms {spread(step['lerp training'])}, peak {peaks['lerp training'] / 2**20:.1f} MiB;  "
                f"cascade / lerp {m['cascade training'] / m['lerp training']:.2f} in time, {peaks['cascade training'] / max(peaks['lerp training'], 1):.2f} in memory")
    del x, g, sections, signals, out, other, gin, kept, fgrads, leaves, leaf_sections, runs
    torch.cuda.empty_cache()


def main():
    global out_file
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="+", default=["10000000:1", f"{1 << 24}:1", f"{1 << 28}:1", "4096:4096"], help="LENGTH:LINES")
    ap.add_argument("--hops", nargs="+", type=int, default=[64, 512, 4096])
    ap.add_argument("--sections", nargs="+", type=int, default=[2, 4, 8])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--signals-below", type=int, default=1 << 62,
                    help="routes (b) and (d) hold 5 K expanded signals and as many gradients: run them for LENGTH * LINES * K below this")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("var2_cascade_frames_probe: needs a GPU")
    if a.out:
        out_file = open(a.out, "w")
    say(f"var2_cascade_frames_probe: {torch.cuda.get_device_name(0)}; steps {a.steps}, rounds {a.rounds}; medians over the rounds (min, max)")
    copy_planes = (torch.rand((4096, 4096), device="cuda"), torch.empty((4096, 4096), device="cuda"))
    for case in a.cases:
        n, lines = (int(v) for v in case.split(":"))
        for hop in a.hops:
            for K in a.sections:
                probe(n, lines, hop, K, a.steps, a.rounds, copy_planes, n * lines * K < a.signals_below)
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
